"""Writes g31_watershed.npz: the labels of tests/watershed_reference.watershed (the heap statement of K28) for

  labels_<name>     the planes of watershed_reference.hand_cases(), made by hand: ties by rank, a ring basin, a basin in a
                    basin, one basin entered from two labels in both orders, a rim pixel claimed directly and through a
                    basin in both orders, a 40-level staircase, the int32 range, negative and large markers
  g28_<name>        the eight (elevation, markers) pairs of g28_fiber_markers.npz
  chain_flooded,    the chained case: g30_clahe.npz's raw channel carried through every stage (its elevation and markers are
  chain_labels      g30's chain_elevation and chain_markers) -- the watershed, and the labels of its class-2 pixels after
                    the CHAIN_MIN_FIBER_SIZE filter (watershed_reference.filtered_labels)

Only results are stored; the inputs come from the reference module and the two older fixtures.  Asserted: the round form
gives the same labels for every case; the basin cases take the basin path and the g28 pairs and the chain do not; the chained
filter keeps a component (chain_largest: the size above which it keeps none).

PXSOM_GOLDEN_OUT: the folder to write to (default: this one)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import watershed_reference as wr  # noqa: E402

CHAIN_MIN_FIBER_SIZE = 15
G28_NAMES, BASIN_CASES = wr.G28_NAMES, wr.BASIN_CASES


def flood(image, markers, name, descent):
    labels, stats = wr.watershed(image, markers), {}
    assert np.array_equal(wr.watershed_rounds(image, markers, stats=stats), labels), name
    assert (stats["descents"] > 0) == descent, (name, stats)
    assert labels.dtype == np.int32 and ((labels != 0).all() or not markers.any()), name
    print("%-26s %3d x %3d  rounds %4d  levels %2d  descents %d" % (name, image.shape[0], image.shape[1], stats["rounds"],
                                                                    stats["levels"], stats["descents"]))
    return labels


def main():
    out_dir = os.environ.get("PXSOM_GOLDEN_OUT", HERE)
    data, hand = {}, wr.hand_cases()
    assert set(BASIN_CASES) <= set(hand)
    for name, (image, markers) in hand.items():
        data["labels_" + name] = flood(image, markers, name, name in BASIN_CASES)
    data["hand_names"] = np.array(json.dumps(list(hand)))
    g28 = np.load(os.path.join(HERE, "g28_fiber_markers.npz"))
    for name in G28_NAMES:
        data["g28_" + name] = flood(g28["elevation_" + name], g28["markers_" + name], "g28 " + name, False)
    g30 = np.load(os.path.join(HERE, "g30_clahe.npz"))
    data["chain_flooded"] = flood(g30["chain_elevation"], g30["chain_markers"], "chain", False)
    chain = wr.filtered_labels(g30["chain_elevation"], g30["chain_markers"], CHAIN_MIN_FIBER_SIZE)
    areas = np.bincount(chain.ravel())[1:]
    assert areas.size and areas.max() >= CHAIN_MIN_FIBER_SIZE, areas
    print("chain filter: components of %s pixels reach %d" % (areas[areas > 0].tolist(), CHAIN_MIN_FIBER_SIZE))
    data["chain_labels"], data["chain_min_fiber_size"] = chain, np.int64(CHAIN_MIN_FIBER_SIZE)
    data["chain_largest"] = np.int64(areas.max())              # a min_fiber_size above this leaves no fibre
    np.savez_compressed(os.path.join(out_dir, "g31_watershed.npz"), **data)


if __name__ == "__main__":
    main()
