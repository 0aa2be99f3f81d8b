"""Randomised parity sweep of K20 pxsom_close_pair_counts (som_device.close_pair_counts) against the numpy statement of
tests/close_pairs_reference.py: number of FOVs (empty ones among them) and their sizes up to 2 000, the two set counts,
the density of the mask bits (stray bits above the set counts included), whether the two masks are one tensor, distlim
and self_neighbor, drawn at random (seeded).  The layouts put pairs at exactly distlim (integer lattices whose pitch
divides it) and cells on one point (clumps).  On every seed compute_mixing_scores is also compared with the loop over
the K13-based create_neighborhood_matrix.  Equality is exact.  ``PXSOM_FUZZ_CASES`` / ``PXSOM_FUZZ_SEED`` as in
test_gpu_fuzz_parity.py.  The generator is device-free (tests/test_mixing.py checks it on CPU)."""
import os

import numpy as np
import pandas as pd
import pytest

from tests import close_pairs_reference as cpr

CASES = int(os.environ.get("PXSOM_FUZZ_CASES", "36"))
SEED = int(os.environ.get("PXSOM_FUZZ_SEED", "20261018"))

LAYOUTS = ["uniform", "lattice", "clumps"]
PHENOTYPES = ["a", "b", "c", "d", "e"]


def gen_case(i, seed=SEED):
    """Case i: dict(xy [n, 2] float64, member_q / member_c [n] uint64 (one object when shared), seg [F + 1] int64,
    n_sets_q, n_sets_c, distlim, self_neighbor, types [n] phenotype names, layout)."""
    rs = np.random.RandomState((seed + 7919 * i) % (2 ** 32))
    layout = LAYOUTS[i % len(LAYOUTS)]
    sizes = [int(rs.choice([0, 1, 2, 63, 64, 65, 255, 256, 257, rs.randint(3, 700), rs.randint(700, 2001)]))
             for _ in range(rs.randint(1, 7))]
    while sum(sizes) > 6000:
        sizes.pop(int(np.argmax(sizes)))
    base = float(rs.choice([10, 37.5, 50]))
    xy = []
    for m in sizes:
        side = max(np.sqrt(m * np.pi * base ** 2 / rs.uniform(2, 30)), base / 4)
        if layout == "lattice":          # an integer lattice whose pitch divides distlim: many pairs at exactly distlim
            pitch = base / rs.choice([2, 5, 10]) if float(base).is_integer() else base / 3
            cols = max(int(np.ceil(np.sqrt(max(m, 1)))), 1)
            idx = rs.permutation(cols * cols)[:m]
            pts = np.stack([idx // cols, idx % cols], 1) * pitch
        elif layout == "clumps":         # groups of coincident cells
            centres = rs.uniform(0, side, (max(m // 8, 1), 2))
            pts = centres[rs.randint(0, len(centres), m)]
        else:
            pts = rs.uniform(0, side, (m, 2))
        xy.append(np.asarray(pts, dtype=np.float64).reshape(m, 2))
    n = int(sum(sizes))
    n_sets_q, n_sets_c = (int(rs.choice([1, 2, 3, 8, 9, 20, 31, 32, 33, 63, 64])) for _ in range(2))

    def masks(density):
        bits = rs.rand(n, 64) < density                   # every bit is drawn: those above the set count are stray
        bits[rs.rand(n) < 0.1] = False                    # cells in no set
        bits[rs.rand(n) < 0.05] = True                    # cells in every set
        return cpr.pack(bits)
    member_q = masks(rs.choice([0.05, 0.3, 0.9]))
    shared = bool(rs.randint(2))
    member_c = member_q if shared else masks(rs.choice([0.05, 0.3, 0.9]))
    distlim = base if rs.randint(2) else (int(base) if float(base).is_integer() else np.float64(base))
    return dict(xy=np.concatenate(xy).reshape(n, 2) if xy else np.zeros((0, 2)), member_q=member_q, member_c=member_c,
                seg=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), n_sets_q=n_sets_q, n_sets_c=n_sets_c,
                distlim=distlim, self_neighbor=bool(rs.randint(2)), types=rs.choice(PHENOTYPES, n), layout=layout)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(CASES))
def test_fuzz_close_pair_counts(gpu, i):
    import torch
    from ark_analysis_amd import som_device
    from ark_analysis_amd.analysis import neighborhood_analysis as na
    from tests import test_mixing as tm
    c = gen_case(i)
    mq = torch.from_numpy(c["member_q"].view(np.int64)).to(gpu)
    mc = mq if c["member_c"] is c["member_q"] else torch.from_numpy(c["member_c"].view(np.int64)).to(gpu)
    got = som_device.close_pair_counts(torch.from_numpy(c["xy"]).to(gpu), mq, mc, torch.from_numpy(c["seg"]).to(gpu),
                                       c["n_sets_q"], c["n_sets_c"], c["distlim"], c["self_neighbor"])
    torch.cuda.synchronize()
    want = cpr.close_pair_counts(c["xy"], c["member_q"], c["member_c"], c["seg"], c["n_sets_q"], c["n_sets_c"],
                                 c["distlim"], c["self_neighbor"])
    got = got.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (c["layout"], c["distlim"], len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])

    if len(c["xy"]) == 0:
        return
    sizes = np.diff(c["seg"])
    table = pd.DataFrame({"fov": np.repeat(["fov%d" % f for f in range(len(sizes))], sizes),
                          "label": np.concatenate([np.arange(1, m + 1) for m in sizes]),
                          "cell_meta_cluster": c["types"], "centroid-0": c["xy"][:, 0], "centroid-1": c["xy"][:, 1]})
    fovs = list(pd.unique(table["fov"]))
    for mixing_type in ("percent", "homogeneous"):
        kwargs = dict(ratio_threshold=3, cell_count_thresh=20)
        scores = na.compute_mixing_scores(table, ["a", "b"], ["c"], mixing_type, distlim=c["distlim"],
                                          self_neighbor=c["self_neighbor"], **kwargs)
        loop = tm.mixing_loop(table, ["a", "b"], ["c"], mixing_type, c["distlim"], c["self_neighbor"], fovs, **kwargs)
        pd.testing.assert_frame_equal(scores, loop, check_exact=True)
