#!/usr/bin/env python3
"""Time of iterative partner matching (gdca_run_partner_ipa_dev) at the pools of DESIGN 3.7's two shapes, species of 1..32
sequences a side from the fixed SplitMix64 stream of tools/partner_bench.py, the first `--rounds` rounds of the loop:
  (a) the device loop: pools, species table, work list, packed pools and the growing alignment resident, scalars alone between rounds;
  (b) the same rounds driven from the host through gdca_run_partner_match with host pointers -- per round the alignment and the pools
      up, match and gap down, the selection in numpy, the next alignment built in numpy: what a caller had to do before the loop
      existed, and the yardstick;
  (c) ms_select a round (the round's figures, its copies and the selection: 28 launches) against the HBM traffic of its passes.
The condition is (a) <= (b): the loop does strictly less (no transfers; the table, the work list and the packed pools once).  The two
are also held to each other bit for bit.  One process; contexts are made before anything is timed; HIP events on the stream the
context works on, 10 timed repeats after 2, medians; every GPU step under a time limit of its own.

    python tools/ipa_bench.py --config B --out profiles/ipa_bench.json   (N = 128, split = 64, K_A = K_B = 4096, n_inc = 256)
    python tools/ipa_bench.py --config C --out profiles/ipa_bench.json   (N = 500, split = 250, K_A = K_B = 8192, n_inc = 512)
Results of several configs are merged into one JSON file by config name."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libgdca.so: INTEGRATION.md "load order")

from partner_bench import PEAK_HBM, species_sizes, step_limit, timed  # noqa: E402

CONFIGS = {"B": dict(N=128, split=64, K=4096, Mfix=256, n_inc=256, theta=0.2, seed=0xB128),
           "C": dict(N=500, split=250, K=8192, Mfix=1024, n_inc=512, theta=-1.0, seed=0xC500)}


def rank_key(x):
    """the ranking's 64-bit key (descending under isless, NaN first, 0.0 before -0.0)"""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    asc = np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))
    return ~np.where(np.isnan(x), np.uint64(0xFFFFFFFFFFFFFFFF), asc)


def select(match, gap, n_take):
    cand = np.nonzero(match >= 0)[0]
    return np.sort(cand[np.argsort(rank_key(gap[cand]), kind="stable")][:max(n_take, 0)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B", choices=sorted(CONFIGS))
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pseudocount", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipa_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 10, "at least 10 timed repeats"

    import gaussdca.jl_amd as gd
    from gaussdca.jl_amd.synth import synth_family

    c = CONFIGS[args.config]
    N, split, K, Mfix, n_inc, q, theta, pc, R = c["N"], c["split"], c["K"], c["Mfix"], c["n_inc"], 21, c["theta"], args.pseudocount, args.rounds
    ENERGY = gd._lib.PAIR_ENERGY
    sizes = species_sizes(K)
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    one = np.nonzero(np.diff(off) == 1)[0]
    seedA = seedB = off[one].astype(np.int32)
    stream = torch.cuda.current_stream()
    with step_limit(60, "contexts"):
        ctx = gd.Context(0, stream=stream.cuda_stream)  # the torch stream: its events time the library's kernels
        torch.cuda.synchronize()
    Zo = synth_family(N, Mfix + K, q, c["seed"])  # (M, N): the first Mfix pairs are known, the others the pools (native pairs, B as it lies)
    Zfix = np.asfortranarray(Zo[:Mfix].T)
    XA, XB = np.asfortranarray(Zo[Mfix:, :split].T), np.asfortranarray(Zo[Mfix:, split:].T)
    with step_limit(60, "upload"):
        dZfix, dXA, dXB = (torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in (Zfix, XA, XB))  # (row k = sequence k: column-major)
        dmatch = torch.empty(K, dtype=torch.int32, device="cuda")
        dgap = torch.empty(K, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
    res = dict(config=args.config, N=N, split=split, KA=K, KB=K, q=q, n=N * (q - 1), Mfix=Mfix, n_seed=int(len(seedA)), n_inc=n_inc, rounds=R,
               theta=theta, pseudocount=pc, repeats=args.repeats, warmup=args.warmup, species=len(sizes))
    last = {}

    def device_loop():
        last["rounds"], last["st"] = ctx.run_partner_ipa_dev(dXA.data_ptr(), K, dXB.data_ptr(), K, off, off, N, q, split, pc, theta,
                                                             dZfix.data_ptr(), Mfix, seedA, seedB, n_inc, R, ENERGY, dmatch.data_ptr(),
                                                             dgap.data_ptr())

    def host_loop():
        Z = np.asfortranarray(np.concatenate([Zfix, np.concatenate([XA[:, seedA], XB[:, seedB]], axis=0)], axis=1))
        sel_before = cand_before = None
        for r in range(1, R + 1):
            (_, m, gp), _ = ctx.run_partner_match_ptr(Z.ctypes.data, N, Z.shape[1], q, pc, theta, split, XA.ctypes.data, K, XB.ctypes.data, K,
                                                      off, off, ENERGY, want_blocks=False)
            last["host_match"], last["host_gap"], last["host_rounds"] = m, gp, r
            a = select(m, gp, r * n_inc)
            if r == R or (r >= 2 and sel_before == cand_before):
                break
            sel_before, cand_before = len(a), int(np.sum(m >= 0))
            Z = np.asfortranarray(np.concatenate([Zfix, np.concatenate([XA[:, a], XB[:, m[a]]], axis=0)], axis=1))

    def keep(key, ms):
        res[key] = statistics.median(ms)
        res[key + "_all"] = ms

    limit = 600 if args.config == "C" else 300
    with step_limit(limit, "(a) the device loop"):
        keep("device_loop_ms", timed(device_loop, args.warmup, args.repeats))
        res["rounds_run"] = len(last["rounds"])
        for k in ("ms_fit", "ms_match", "ms_select"):
            res[k + "_per_round"] = statistics.median(rd[k] for rd in last["rounds"])
        res["M_train"] = [int(rd["M_train"]) for rd in last["rounds"]]
        match_dev, gap_dev = dmatch.cpu().numpy(), dgap.cpu().numpy()
    with step_limit(limit, "(b) the host-driven loop"):
        keep("host_loop_ms", timed(host_loop, args.warmup, args.repeats))
    ctx.close()
    res["loop_equals_host_driven"] = bool(last["host_rounds"] == res["rounds_run"] and np.array_equal(match_dev, last["host_match"]) and
                                          np.array_equal(gap_dev.view(np.uint64), last["host_gap"].view(np.uint64)))
    res["glue_ms_saved_per_round"] = (res["host_loop_ms"] - res["device_loop_ms"]) / max(res["rounds_run"], 1)
    # (c) the selection's traffic: the key kernel (12 K read, 12 K written), eight passes of histogram (8 K read) and scatter (12 K read,
    # 12 K written), the flags (4 K read, 4 K written), the compaction (8 K read, 4 K written); the round's figures and the copies of
    # match and gap (~50 K more).  At K of a few thousand that is some microseconds of HBM time: the stage is its 28 launches.
    res["select_bytes"] = float(K) * (24 + 8 * 32 + 8 + 12 + 50)
    res["select_hbm_ms_at_peak"] = res["select_bytes"] / PEAK_HBM * 1e3
    res["select_launches"] = 28
    res["condition_device_le_host"] = bool(res["device_loop_ms"] <= res["host_loop_ms"])

    allres = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            allres = json.load(f)
    allres[args.config] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(allres, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_all")}, sort_keys=True))
    sys.exit(0 if res["condition_device_le_host"] and res["loop_equals_host_driven"] else 1)


if __name__ == "__main__":
    main()
