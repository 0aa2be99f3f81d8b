"""Prints one case of a generator of tests/test_gpu_fuzz_preprocessing.py (test tooling, device-free): its class, its
scalar parameters and the shape, dtype and value summary of every array -- what a failing test's tag names.
python -m tests.tools.replay_preprocessing_case <family> <case index>     (families: see FAMILIES in that file)"""
import sys

import numpy as np

from tests.test_gpu_fuzz_preprocessing import FAMILIES, SEED


def _show(key, value, indent="  "):
    if isinstance(value, np.ndarray):
        line = "%s%s: %s %s" % (indent, key, value.dtype, value.shape)
        if value.size and value.dtype.kind == "f":
            with np.errstate(all="ignore"):
                f = value[np.isfinite(value)].astype(np.float64)
                line += " finite min %r max %r, %d NaN, %d inf, %d zero" % (
                    float(f.min()) if f.size else None, float(f.max()) if f.size else None, int(np.isnan(value).sum()),
                    int(np.isinf(value).sum()), int((value == 0).sum()))
        elif value.size:
            line += " min %d max %d" % (int(value.min()), int(value.max()))
        print(line)
    elif isinstance(value, list):
        for j, item in enumerate(value):
            print("%s%s[%d]:" % (indent, key, j))
            for k, v in item.items():
                _show(k, v, indent + "    ")
    else:
        print("%s%s: %r" % (indent, key, value))


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] not in FAMILIES:
        sys.exit(__doc__ + "\nfamilies: " + ", ".join(sorted(FAMILIES)))
    gen, salt, classes = FAMILIES[sys.argv[1]]
    target = int(sys.argv[2])
    case = list(gen(SEED + salt, target + 1))[target]
    print("%s case %d of seed %d (PXSOM_FUZZ_SEED=%d): class %s of %d" % (
        sys.argv[1], target, SEED + salt, SEED, case["cls"], len(classes)))
    for key, value in case.items():
        _show(key, value)
