#!/usr/bin/env python3
"""Device time of the replica-exchange chains (k_temper.hip) against the plain Metropolis chains (k_sample.hip) at the same number of
workgroups and proposals: K = 256 chains of R = 8 replicas, swap_every = N, on a resident mJ from random residue sequences --
gdca_sample_tempered_dev over a geometric ladder from beta = 1 -- against gdca_sample_dev running K R plain chains for the same
n_steps at the ONE beta that reproduces the ladder's mean acceptance (found by bisection on the plain chains: the acceptance falls
with beta).  gdca_sample_dev is code the tempered chains do not touch.  Reported: both times (medians of 10 after 2 warm-ups, HIP
events on the stream the context works on; each includes its start tables, the tempered one its start energies too), their ratio,
the run-to-run spread of the plain figure, and the estimate from bytes: the tempered replicas reload and write back their tables
once a round (2 x 8 N s bytes a replica and round where the table lives in LDS) where the plain chains do so once a call, against
the two columns of mJ an accepted move reads (16 n bytes).  Every GPU step runs under a time limit of its own.

    python tools/temper_bench.py --config B --out profiles/temper_bench.json   (N = 128, M = 10 000)
    python tools/temper_bench.py --config C --out profiles/temper_bench.json   (N = 500, M = 50 000)
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

from mutation_bench import CONFIGS, FN_HBM_FRACTION, PEAK_HBM, step_limit, timed  # noqa: E402

K, R = 256, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B", choices=sorted(CONFIGS))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweeps", type=int, default=16, help="n_steps = sweeps N, one round a sweep")
    ap.add_argument("--beta-min", type=float, default=0.3, help="the ladder is geometric from 1 down to this")
    ap.add_argument("--pseudocount", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temper_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 10, "at least 10 timed repeats"

    import gaussdca.jl_amd as gd
    from gaussdca.jl_amd import devops
    from gaussdca.jl_amd.synth import synth_family

    c = CONFIGS[args.config]
    N, M, q, theta, pc = c["N"], c["M"], 21, c["theta"], args.pseudocount
    s = q - 1
    n, G, T = N * s, K * R, args.sweeps * N
    betas = [float(b) for b in np.geomspace(1.0, args.beta_min, R)]
    stream = torch.cuda.current_stream()
    with step_limit(60, "contexts"):
        ctx = gd.Context(0, stream=stream.cuda_stream)  # the torch stream: its events time the library's kernels
        torch.cuda.synchronize()
    Zo = synth_family(N, M, q, c["seed"])  # (M, N)
    X = np.random.default_rng(c["seed"]).integers(1, q, size=(G, N)).astype(np.int8)  # (G, N) rows = N x R x K column-major; residues only
    with step_limit(60, "upload"):
        dZ = torch.from_numpy(Zo).cuda()
        dX = torch.from_numpy(X).cuda()
        dXs = torch.empty((G, N), dtype=torch.int8, device="cuda")
        dXo = torch.empty((G, N), dtype=torch.int8, device="cuda")
        dacc = torch.empty(G, dtype=torch.int32, device="cuda")
        dsw = torch.empty(K * (R - 1), dtype=torch.int32, device="cuda")
        dso = torch.empty(G, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
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

    def tempered(ladder=betas):  # one sample, behind the last round
        ctx.sample_tempered_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dX.data_ptr(), None, K, ladder, None, 0, 1, 0, N, T - N, N, 1, dXs.data_ptr(),
                                dacc.data_ptr(), dsw.data_ptr(), dXo.data_ptr(), dso.data_ptr())

    def plain(beta):
        ctx.sample_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dX.data_ptr(), G, None, 0, beta, 1, 0, T - 1, 1, 1, dXs.data_ptr(), dacc.data_ptr())

    def acceptance():
        return float(dacc.cpu().numpy().astype(np.int64).sum()) / (G * T)

    with step_limit(600, "tempered chains"):
        ms_t = timed(tempered, args.warmup, args.repeats)
        acc_slot = dacc.cpu().numpy().astype(np.int64).reshape(K, R).sum(axis=0) / (K * T)
        rounds = T // N
        att = np.array([(rounds - p % 2 + 1) // 2 for p in range(R - 1)], dtype=np.float64)
        swap_rate = dsw.cpu().numpy().astype(np.int64).reshape(K, R - 1).sum(axis=0) / (K * att)
        mean_acc = float(acc_slot.mean())
    with step_limit(600, "the plain chains' beta"):
        lo, hi = 0.0, 4.0  # the acceptance falls with beta: bisect on the plain chains themselves
        for _ in range(12):
            mid = (lo + hi) / 2
            plain(mid)
            ctx.synchronize()
            lo, hi = (mid, hi) if acceptance() > mean_acc else (lo, mid)
        beta_eq = (lo + hi) / 2
    with step_limit(600, "plain chains"):
        ms_p = timed(lambda: plain(beta_eq), args.warmup, args.repeats)
        acc_p = acceptance()
    with step_limit(600, "tempered chains, one temperature"):
        # every slot at the plain chains' beta: the launch structure alone (a launch a round, the tables reloaded, every round waiting
        # for its slowest workgroup) without the ladder's unequal acceptance -- what separates the two parts of the gap
        ms_e = timed(lambda: tempered([beta_eq] * R), args.warmup, args.repeats)
        acc_e = acceptance()
    with step_limit(240, "start tables and energies"):
        dD = torch.empty(G * N * q, dtype=torch.float64, device="cuda")
        dE = torch.empty(G, dtype=torch.float64, device="cuda")
        ms_scan = timed(lambda: ctx.mutation_scan_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dX.data_ptr(), G, gd._lib.MUT_POTENTIAL, dD.data_ptr()),
                        args.warmup, args.repeats)
        ms_en = timed(lambda: ctx.energies_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dX.data_ptr(), G, dE.data_ptr()), args.warmup, args.repeats)
    ctx.close()

    t, p = statistics.median(ms_t), statistics.median(ms_p)
    lds_table = bool(8 * (4 + N * q) + 32 + 2 * N <= 160 * 1024)
    hbm = [f * PEAK_HBM for f in FN_HBM_FRACTION]
    table_bytes = 2.0 * 8 * N * s * G * (rounds - 1) if lds_table else 0.0  # what the plain chains do once, the tempered ones once a round
    move_bytes = 16.0 * n * mean_acc * G * T
    res = dict(config=args.config, N=N, M=M, q=q, n=n, K=K, R=R, swap_every=N, n_steps=T, rounds=rounds, betas=betas, repeats=args.repeats,
               warmup=args.warmup, sequences="uniformly random residues, no gaps", flags=0, table_in_lds=lds_table,
               tempered_ms=t, tempered_ms_all=ms_t, acceptance_by_slot=acc_slot.tolist(), mean_acceptance=mean_acc, swap_rate_by_pair=swap_rate.tolist(),
               plain_beta=beta_eq, plain_acceptance=acc_p, plain_ms=p, plain_ms_all=ms_p, plain_spread=(max(ms_p) - min(ms_p)) / p,
               ratio=t / p, tempered_one_beta_ms=statistics.median(ms_e), tempered_one_beta_ms_all=ms_e, tempered_one_beta_acceptance=acc_e,
               ratio_one_beta=statistics.median(ms_e) / p, scan_ms=statistics.median(ms_scan), energies_ms=statistics.median(ms_en),
               launches_tempered=2 * rounds + 2, extra_table_bytes=table_bytes, accepted_move_bytes=move_bytes,
               extra_table_ms_at_hbm_rate=[table_bytes / f * 1e3 for f in hbm], accepted_move_ms_at_hbm_rate=[move_bytes / f * 1e3 for f in hbm],
               estimated_ratio_from_bytes=1.0 + table_bytes / move_bytes if move_bytes else None)
    print("config %s: tempered %.3f ms, plain at beta %.4f %.3f ms (acceptance %.4f / %.4f), ratio %.3f, plain spread %.3f, bytes estimate %.3f"
          % (args.config, t, beta_eq, p, mean_acc, acc_p, t / p, res["plain_spread"], res["estimated_ratio_from_bytes"] or 0.0), flush=True)
    print("config %s: tempered with every slot at beta %.4f: %.3f ms, ratio %.3f" % (args.config, beta_eq, res["tempered_one_beta_ms"],
                                                                                  res["ratio_one_beta"]), flush=True)
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
