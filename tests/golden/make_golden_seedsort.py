"""Search for key arrays on which the seeding stage's instance of the wave sort (wave_sort_kv<12, 32, 12>, smg_wsort.hpp) flushes
its list of short ranges in the middle of the recursion: at most 255 keys whose quicksort recursion (sort.c:233) reaches more than
32 ranges of 2..32 keys.  Sorted, reversed, organ-pipe, constant and random arrays give 8 to 19.  A seeded annealing over
permutations of n distinct keys, scored by oracle/or_seed.c: or_sort_listed_ranges; the arrays found go to
tests/golden/seedsort_adversaries.json (data only; tests/seed_ref.py: listed_ranges restates the count in Python).
usage: python tests/golden/make_golden_seedsort.py [proposals per run]"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as ol  # noqa: E402


def score(a, buf):
    buf[:] = a
    return ol.lib().or_sort_listed_ranges(a.size, buf.ctypes.data)


def anneal(n, seed, proposals, want=None):
    """-> (best array, its count); stops early at a count of exactly `want`"""
    rng = np.random.default_rng(seed)
    a = rng.permutation(n).astype(np.uint32)
    buf = np.zeros(n, np.uint32)
    cur = score(a, buf)
    best, best_a = cur, a.copy()
    ij = rng.integers(0, n, size=(proposals, 2))
    u = rng.random(proposals)
    for t in range(proposals):
        i, j = int(ij[t, 0]), int(ij[t, 1])
        if i == j:
            continue
        a[i], a[j] = a[j], a[i]
        sc = score(a, buf)
        temp = 0.6 * (1.0 - t / proposals) + 0.02
        if sc >= cur or u[t] < np.exp((sc - cur) / temp):
            cur = sc
            if cur > best:
                best, best_a = cur, a.copy()
            if want is not None and cur == want:
                return a.copy(), cur
        else:
            a[i], a[j] = a[j], a[i]
    return best_a, best


def main():
    proposals = int(sys.argv[1]) if len(sys.argv) > 1 else 1500000
    ol.lib().or_sort_listed_ranges.argtypes = [ol.C.c_int, ol.C.c_void_p]
    out = []
    for n, seed in ((255, 1), (255, 2), (254, 3), (250, 4)):
        a, sc = anneal(n, seed, proposals)
        print("n %d seed %d: %d listed ranges" % (n, seed, sc), flush=True)
        out.append(dict(n=n, seed=seed, ranges=int(sc), keys=[int(x) for x in a]))
    a, sc = anneal(255, 5, proposals, want=32)
    print("n 255 seed 5, stopping at 32: %d listed ranges" % sc, flush=True)
    out.append(dict(n=255, seed=5, ranges=int(sc), keys=[int(x) for x in a]))
    with open(os.path.join(HERE, "seedsort_adversaries.json"), "w") as f:
        json.dump(dict(proposals=proposals, arrays=out), f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
