"""The communicators libpxsom owns: RCCL (RankComm) and one-shot peer-to-peer over HIP IPC (P2PComm)."""
import ctypes

import torch

from .. import _capi


class _Comm:
    """What both communicators do with their ``handle``: the sum all-reduce and the release."""

    def allreduce_sum(self, t: torch.Tensor) -> None:
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("the exchange reduces contiguous float64 buffers")
        _capi.call("pxsom_comm_allreduce_sum_f64", self.handle, t.data_ptr(), t.numel(), _capi.stream_ptr())

    def close(self) -> None:
        if self.handle is not None:
            h, self.handle = self.handle, None
            _capi.call("pxsom_comm_destroy", h)


COMM_ID_BYTES = 128  # include/pxsom.h PXSOM_COMM_ID_BYTES


def _torch_rccl_path() -> str:
    """The librccl.so this process already uses: PyTorch's own copy (binding a second RCCL next to it is
    what pxsom_comm_bind exists to avoid); empty = let the library fall back to the system one."""
    import os
    override = os.environ.get("PXSOM_RCCL_LIBRARY")     # another build of the collective library (tests: a stand-in)
    if override:
        return override
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
    return path if os.path.exists(path) else ""


class RankComm(_Comm):
    """RCCL communicator owned by libpxsom (pxsom_comm_*): what the in-library exchange of a multi-rank batch
    run reduces over.  ``RankComm.unique_id()`` on one rank, the 128 bytes handed to the others by the
    launcher's channel, then ``RankComm(id, nranks, rank)`` on every rank (collective) with its device current."""

    def __init__(self, uid: bytes, nranks: int, rank: int):
        self.bind()
        if len(uid) != COMM_ID_BYTES:
            raise ValueError("communicator id must be %d bytes" % COMM_ID_BYTES)
        box = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(bytes(uid), COMM_ID_BYTES)
        _capi.call("pxsom_comm_create", ctypes.cast(buf, ctypes.c_void_p), COMM_ID_BYTES, int(nranks), int(rank),
                   ctypes.byref(box))
        self.handle = box
        self.nranks, self.rank = int(nranks), int(rank)

    @staticmethod
    def bind() -> None:
        _capi.call("pxsom_comm_bind", _torch_rccl_path().encode())

    @staticmethod
    def unique_id() -> bytes:
        RankComm.bind()
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        _capi.call("pxsom_comm_unique_id", ctypes.cast(buf, ctypes.c_void_p), COMM_ID_BYTES)
        return buf.raw


P2P_HANDLE_BYTES = 64  # include/pxsom.h PXSOM_P2P_HANDLE_BYTES


class P2PComm(_Comm):
    """One-shot peer-to-peer exchange owned by libpxsom (pxsom_comm_p2p_*): every rank's block of device memory is mapped
    by the others through HIP IPC, an all-reduce is one launch per rank and gives bit-identical sums on all ranks.  Ranks
    may share a device.  Two phases, so that a launcher can agree on each before the next: the constructor allocates the
    own block (``local_handle``: 64 bytes), ``connect`` takes the handles of all ranks in rank order (``gather``: a
    callable doing both in one go, e.g. over ``torch.distributed.all_gather_object``).  Same interface as RankComm."""

    def __init__(self, nranks: int, rank: int, max_count: int, gather=None):
        box = ctypes.c_void_p()
        _capi.call("pxsom_comm_p2p_create", int(nranks), int(rank), int(max_count), ctypes.byref(box))
        self.handle = box
        self.nranks, self.rank, self.max_count = int(nranks), int(rank), int(max_count)
        self.fused = False
        mine = ctypes.create_string_buffer(P2P_HANDLE_BYTES)
        _capi.call("pxsom_comm_p2p_handle", self.handle, ctypes.cast(mine, ctypes.c_void_p), P2P_HANDLE_BYTES)
        self.local_handle = mine.raw          # 64 bytes: what the other ranks need to map this rank's block
        if gather is not None:
            self.connect(gather(self.local_handle))

    def connect(self, handles) -> None:
        """Maps the blocks of all ranks (``handles``: every rank's ``local_handle``, rank order)."""
        handles = list(handles)
        if len(handles) != self.nranks or any(len(h) != P2P_HANDLE_BYTES for h in handles):
            raise ValueError("one %d-byte handle per rank, in rank order" % P2P_HANDLE_BYTES)
        blob = ctypes.create_string_buffer(b"".join(handles), P2P_HANDLE_BYTES * self.nranks)
        _capi.call("pxsom_comm_p2p_connect", self.handle, ctypes.cast(blob, ctypes.c_void_p),
                   P2P_HANDLE_BYTES * self.nranks)

    def set_fused(self, on: bool) -> None:
        """The fused 10 x 10 training step runs the exchange inside its own launch (every rank: the same value)."""
        _capi.call("pxsom_comm_p2p_set_fused", self.handle, 1 if on else 0)
        self.fused = bool(on)

    def error_epoch(self) -> int:
        """0, or the number of the first exchange a peer did not arrive at in time (its result was NaN)."""
        out = ctypes.c_uint64(0)
        _capi.call("pxsom_comm_p2p_error", self.handle, ctypes.byref(out))
        return int(out.value)
