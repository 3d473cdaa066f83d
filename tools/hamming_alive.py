"""Where does the three-plane Hamming bound decide?  (numpy only, no GPU.)

For sampled pairs of a synthetic family -- the benchmark's own generator, tests/host_mirrors.synth_family_py -- the fraction
still ALIVE after w words of 32 positions: partial distance on the three low bit planes below thresh = floor(theta N), theta
as the library computes it (compute_theta's :auto rule, or the configuration's fixed theta).  This is what k_hamming's probe
counts on its sampled tiles and what csrc/gdca_hamming_cut.h picks the cut word from.

    python tools/hamming_alive.py [--config C] [--pairs 3000000]
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
    low[:, :N] = Z & 7
    rng = np.random.default_rng(1)
    alive = np.zeros(NW, dtype=np.int64)
    done = 0
    while done < args.pairs:
        n = min(200_000, args.pairs - done)
        k, l = rng.integers(0, M, n), rng.integers(0, M, n)
        keep = k != l
        k, l = k[keep], l[keep]
        diff = (low[k] != low[l]).reshape(len(k), NW, 32).sum(axis=2)
        part = np.cumsum(diff, axis=1)
        alive += (part < thresh).sum(axis=0)
        done += len(k)
    print("config %s: N = %d, M = %d, thresh = %d, NW = %d, %d sampled pairs" % (args.config, N, M, thresh, NW, done))
    print("  w  alive fraction after w words   expected entries of a 128 x 128 tile's lists")
    for w in range(1, NW + 1):
        a = alive[w - 1] / done
        print("%3d  %.3e                      %9.1f" % (w, a, a * 16384))


if __name__ == "__main__":
    main()
