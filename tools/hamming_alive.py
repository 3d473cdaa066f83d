"""Where does a lower bound of the Hamming distance decide?  (numpy only, no GPU.)

For sampled pairs of a synthetic family -- the benchmark's own generator, tests/host_mirrors.synth_family_py -- the fraction
still ALIVE after w words of 32 positions: partial distance on the three low bit planes below thresh = floor(theta N), theta
as the library computes it (compute_theta's :auto rule, or the configuration's fixed theta).  This is what k_hamming's probe
counts on its sampled tiles and what csrc/gdca_hamming_cut.h picks the cut word from.

--bound consensus: the one-plane bound of csrc/k_hamming_fp4.hip instead -- a position counts where exactly one of the two
sequences carries its column's most frequent symbol (ties to the smallest symbol, as k_fp4_sigma breaks them).  The last row is
the fraction of pairs the form lists; the summary line sets it beside the true neighbours and the three-plane bound's list.

    python tools/hamming_alive.py [--config C] [--pairs 3000000] [--bound three-plane|consensus]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = {"B": (128, 10000, 0.2, 0xB128), "C": (500, 50000, -1.0, 0xC500), "D": (1000, 100000, -1.0, 0xD1000)}


def auto_theta(Z):
    """compute_theta (:auto) -- the oracle's statement of it"""
    from oracle import gdca_oracle as o

    return float(o.compute_theta(Z))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C", choices=sorted(CONFIGS))
    ap.add_argument("--pairs", type=int, default=3_000_000)
    ap.add_argument("--thresh", type=int, default=0, help="override floor(theta N)")
    ap.add_argument("--bound", default="three-plane", choices=("three-plane", "consensus"))
    args = ap.parse_args()
    from host_mirrors import synth_family_py

    N, M, theta, seed = CONFIGS[args.config]
    Z = synth_family_py(N, M, 21, seed)  # (M, N) int8
    if args.thresh:
        thresh = args.thresh
    else:
        th = theta if theta >= 0 else auto_theta(Z)
        thresh = int(np.floor(th * N))
    NW = (N + 31) // 32
    low = np.zeros((M, NW * 32), dtype=np.uint8)
    if args.bound == "consensus":
        sigma = np.array([np.bincount(Z[:, i] & 31, minlength=32).argmax() for i in range(N)], dtype=np.uint8)  # (argmax: the first maximum)
        low[:, :N] = (Z & 31) != sigma
    else:
        low[:, :N] = Z & 7
    full = np.zeros((M, NW * 32), dtype=np.uint8)
    full[:, :N] = Z
    rng = np.random.default_rng(1)
    alive = np.zeros(NW, dtype=np.int64)
    true_n = low3_n = 0
    done = 0
    while done < args.pairs:
        n = min(200_000, args.pairs - done)
        k, l = rng.integers(0, M, n), rng.integers(0, M, n)
        keep = k != l
        k, l = k[keep], l[keep]
        diff = (low[k] != low[l]).reshape(len(k), NW, 32).sum(axis=2)
        part = np.cumsum(diff, axis=1)
        alive += (part < thresh).sum(axis=0)
        true_n += int(((full[k] != full[l]).sum(axis=1) < thresh).sum())
        low3_n += int((((full[k] & 7) != (full[l] & 7)).sum(axis=1) < thresh).sum())
        done += len(k)
    print("config %s: N = %d, M = %d, thresh = %d, NW = %d, %d sampled pairs, bound: %s" % (args.config, N, M, thresh, NW, done, args.bound))
    print("  fraction of pairs below thresh: true distance %.3e, three-plane bound %.3e, this bound %.3e" % (true_n / done, low3_n / done, alive[-1] / done))
    print("  w  alive fraction after w words   expected entries of a 128 x 128 tile's lists")
    for w in range(1, NW + 1):
        a = alive[w - 1] / done
        print("%3d  %.3e                      %9.1f" % (w, a, a * 16384))


if __name__ == "__main__":
    main()
