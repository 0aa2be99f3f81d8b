"""ark_analysis_amd -- MI355X (gfx950) implementation of ark-analysis' Pixie pixel/cell SOM hot path.

Layout
  csrc/ + include/pxsom.h   hand-written HIP kernels behind a C ABI (libpxsom.so)
  _capi                      ctypes binding: the prototype table, ``check`` / ``call`` of a status-returning entry
  som_device/                torch-tensor plumbing, one module per kernel family (_args: the shared checks; som, comm,
                             pixels, planes, cells, spatial, clustering); every name is reached as ``som_device.NAME``
  flowsom                    pyFlowSOM-compatible ``som`` / ``map_data_to_nodes`` (the two foreign
                             calls the reference makes, cluster_helpers.py:106-109, 152-157)
  distributed                FOV-sharded batch SOM training with per-step RCCL all-reduce
  phenotyping/               mirrors of the reference's pipeline modules (same names/signatures)

(The directory is ``ark_analysis_amd`` rather than ``ark-analysis_amd`` because a Python package
name cannot contain a hyphen.)
"""
__version__ = "0.1.0"
