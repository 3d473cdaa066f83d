#!/usr/bin/env python3
"""Device time of the Metropolis chains (k_sample.hip) at two shapes and K = 1, 256, 8192 chains from random residue sequences on a
resident mJ: gdca_sample_dev at beta = 0.5, 1, 2 -- ns per proposal, ns per accepted move, the acceptance rate --, at beta = 0 (every
proposal accepted: the cost of an accepted move) and at beta = 1e9 (once a chain sits in a local minimum nothing is accepted: the
cost of a rejected proposal), one launch of GDCA_SAMPLE_CHUNK_RULE proposals (K = 256), against the floors of an accepted move of
section 3.8b -- two columns of 8 n bytes at the HBM rate k_fn20 reaches, the table's 2 N s accesses of 8 bytes in LDS -- and against
what a caller had to do for one proposal before: gdca_mutation_scan_dev, a download of D, the decision in numpy and an upload of the
changed sequences.  One process; HIP events on the stream the context works on for the device calls, the host clock around the old
route; every GPU step under a time limit of its own (a step that overruns ends the process with status 124).

    python tools/sample_bench.py --config B --out profiles/sample_bench.json   (N = 128, M = 10 000)
    python tools/sample_bench.py --config C --out profiles/sample_bench.json   (N = 500, M = 50 000)
Results of several configs are merged into one JSON file by config name."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libgdca.so: INTEGRATION.md "load order")

from mutation_bench import CONFIGS, CUS, FN_HBM_FRACTION, GHZ, KS, LDS_BYTES_PER_CLK, PEAK_HBM, step_limit, timed  # noqa: E402

BETAS = (0.5, 1.0, 2.0)
CHUNK = 65536  # GDCA_SAMPLE_CHUNK_RULE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C", choices=sorted(CONFIGS))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--old-steps", type=int, default=5, help="timed proposals of the old route (one more runs first, untimed)")
    ap.add_argument("--pseudocount", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 10, "at least 10 timed repeats"

    import gaussdca.jl_amd as gd
    from gaussdca.jl_amd import devops
    from gaussdca.jl_amd.synth import synth_family

    c = CONFIGS[args.config]
    N, M, q, theta, pc = c["N"], c["M"], 21, c["theta"], args.pseudocount
    s = q - 1
    n = N * s
    stream = torch.cuda.current_stream()
    with step_limit(60, "contexts"):
        ctx = gd.Context(0, stream=stream.cuda_stream)  # the torch stream: its events time the library's kernels
        torch.cuda.synchronize()
    Zo = synth_family(N, M, q, c["seed"])  # (M, N)
    KMAX = max(KS)
    X = np.random.default_rng(c["seed"]).integers(1, q, size=(KMAX, N)).astype(np.int8)  # (K, N) rows = N x K column-major; residues only
    with step_limit(60, "upload"):
        dZ = torch.from_numpy(Zo).cuda()
        dX = torch.from_numpy(X).cuda()
        dD = torch.empty(KMAX * N * q, dtype=torch.float64, device="cuda")
        dXs = torch.empty((KMAX, N), dtype=torch.int8, device="cuda")
        dacc = torch.empty(KMAX, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
    res = dict(config=args.config, N=N, M=M, q=q, n=n, theta=theta, pseudocount=pc, repeats=args.repeats, warmup=args.warmup,
               old_route_steps=args.old_steps, sequences="uniformly random residues, no gaps", flags=0, K={})

    with step_limit(180, "operator chain"):
        dPi = torch.empty(n, dtype=torch.float64, device="cuda")
        dmJ = torch.empty(n * n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        dW, Meff, _, _ = devops.compute_weights_dev(ctx, dZ.data_ptr(), N, M, theta if theta >= 0 else ":auto")
        devops.compute_weighted_frequencies_dev(ctx, dZ.data_ptr(), N, M, q, dW, Meff, dPi.data_ptr(), dmJ.data_ptr())
        devops.add_pseudocount_dev(ctx, dPi.data_ptr(), dmJ.data_ptr(), N, q, pc)
        devops.compute_C_dev(ctx, dPi.data_ptr(), dmJ.data_ptr(), n, dC=dmJ.data_ptr())
        devops.inv_cholesky_dev(ctx, dmJ.data_ptr(), n)
        ctx.synchronize()

    def chains(K, beta, T):  # one sample, behind the last proposal
        ctx.sample_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dX.data_ptr(), K, None, 0, beta, 1, 0, T - 1, 1, 1, dXs.data_ptr(), dacc.data_ptr())

    hbm_rate = [f * PEAK_HBM for f in FN_HBM_FRACTION]
    lds_rate = CUS * GHZ * 1e9 * LDS_BYTES_PER_CLK
    for K in KS:
        r = {}
        T = 4096 if K <= 256 else 1024
        r["n_steps"] = T
        with step_limit(240, "scan K=%d" % K):
            ms = timed(lambda: ctx.mutation_scan_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dX.data_ptr(), K, gd._lib.MUT_POTENTIAL, dD.data_ptr()),
                       args.warmup, args.repeats)
            r["scan_ms"] = statistics.median(ms)  # the stage's first part, and the old route's device part
        for beta in (0.0,) + BETAS + (1e9,):
            key = "beta_%g" % beta
            with step_limit(600, "gdca_sample_dev K=%d beta=%g" % (K, beta)):
                ms = timed(lambda: chains(K, beta, T), args.warmup, args.repeats)
                acc = dacc[:K].cpu().numpy().astype(np.int64)
            kern = statistics.median(ms) - r["scan_ms"]  # the chains alone
            total_acc = float(acc.sum())
            e = dict(ms=statistics.median(ms), ms_all=ms, acceptance=total_acc / (K * T), accepted_mean=float(acc.mean()),
                     ns_per_proposal_and_chain=kern * 1e6 / (K * T), ns_per_proposal_of_the_batch=kern * 1e6 / T)
            if total_acc:
                e["ns_per_accepted_move_and_chain"] = kern * 1e6 / total_acc
                # floors of the accepted moves alone (3.8b's): two columns of 8 n bytes a move from HBM; the table's N s entries read and written
                hbm = [16.0 * n * total_acc / f * 1e3 for f in hbm_rate]
                lds = 16.0 * N * s * total_acc / (lds_rate * min(K, CUS) / CUS) * 1e3
                e["floor_hbm_ms"], e["floor_lds_ms"] = hbm, lds
                e["floor_binds"] = "hbm" if min(hbm) >= lds else "lds"
                e["floor_fraction"] = max(min(hbm), lds) / kern
            r[key] = e
        r["lds_table"] = bool(8 * (4 + N * q) + 32 + 2 * N <= 160 * 1024)
        if K == 256:  # one launch of the rule's length
            with step_limit(600, "one launch of %d proposals" % CHUNK):
                ms = timed(lambda: chains(K, 1.0, CHUNK), 1, 3)
            r["launch_of_rule_length_ms"] = statistics.median(ms) - r["scan_ms"]
            r["launch_of_rule_length_ms_all"] = ms

        # ---- the old route, one proposal a chain: scan (delta), download, the decision on the host, upload of the changed sequences
        with step_limit(600, "old route K=%d" % K):
            rng = np.random.default_rng(K)
            Xh = X[:K].copy()
            dXo = torch.from_numpy(Xh).cuda()
            rows = np.arange(K)
            ts = []
            for it in range(args.old_steps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.mutation_scan_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dXo.data_ptr(), K, gd._lib.MUT_DELTA, dD.data_ptr())
                D = dD[:K * N * q].view(K, N, q).cpu().numpy()
                i = rng.integers(0, N, size=K)
                v = rng.integers(0, s - 1, size=K)
                b = v + (v >= Xh[rows, i] - 1)
                go = 1.0 * D[rows, i, b] <= -np.log(1.0 - rng.random(K))
                Xh[rows[go], i[go]] = (b[go] + 1).astype(np.int8)
                dXo.copy_(torch.from_numpy(Xh))
                torch.cuda.synchronize()
                if it:
                    ts.append((time.perf_counter() - t0) * 1e3)
            r["old_route_ms_per_proposal"] = statistics.median(ts)
            r["old_route_ms_per_proposal_all"] = ts
            del D
        r["speedup_per_proposal_beta_1"] = r["old_route_ms_per_proposal"] / (r["beta_1"]["ms"] / T)  # (the chains' scan included)
        res["K"][str(K)] = r
        print("K %5d: " % K + ", ".join("beta %g: %.1f ns a proposal and chain, acceptance %.3f" % (bt, r["beta_%g" % bt]["ns_per_proposal_and_chain"],
                                                                                             r["beta_%g" % bt]["acceptance"])
                                        for bt in (0.0,) + BETAS + (1e9,)) +
              "; old route %.3f ms a proposal, speedup %.0f" % (r["old_route_ms_per_proposal"], r["speedup_per_proposal_beta_1"]), flush=True)
    ctx.close()

    allres = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            allres = json.load(f)
    allres[args.config] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(allres, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
