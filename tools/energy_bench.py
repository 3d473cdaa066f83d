#!/usr/bin/env python3
"""Device time of the energy stage (k_energy.hip) at bench.py's synthetic families: alone on a resident mJ (gdca_energies_dev), as
ms_score of the fused run (gdca_run_energies_dev), against its two rooflines, against the obvious torch formulation on the same GPU,
and the fused run's ms_total beside a plain gdca_run's.  One process; contexts are made before anything is timed (as bench.py does);
HIP events on the stream the context works on; every GPU step under a time limit of its own (a step that overruns ends the process
with status 124, nothing is started after it).

    python tools/energy_bench.py --config C --out profiles/energy_bench.json     (N = 500, q = 21, K = M = 50 000)
    python tools/energy_bench.py --config B --out profiles/energy_bench.json     (N = 128, M = 10 000)
Results of several configs are merged into one JSON file by config name."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libgdca.so: INTEGRATION.md "load order")
import numpy as np  # noqa: E402

CONFIGS = {"B": dict(N=128, M=10000, theta=0.2, seed=0xB128), "C": dict(N=500, M=50000, theta=-1.0, seed=0xC500)}
PEAK_HBM = 8.0e12                  # bytes / s
FN_HBM_FRACTION = (0.58, 0.64)     # what k_fn20 reaches on the same triangle
CUS, GHZ, LDS_B64_PER_CLK = 256, 2.4, 32  # ds_read_b64: 256 B / clk / CU, conflict-free


@contextlib.contextmanager
def step_limit(seconds, what):
    def over():
        sys.stderr.write("energy_bench: step '%s' exceeded %d s\n" % (what, seconds))
        sys.stderr.flush()
        os._exit(124)

    t = threading.Timer(seconds, over)
    t.daemon = True
    t.start()
    try:
        yield
    finally:
        t.cancel()


def timed(fn, warmup, repeats):
    """HIP events on the current torch stream (the context was made on it) -> list of ms"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def torch_energies(mJz, g, c0, idx, chunk):
    """the obvious formulation: gather the N x N entries of every sequence and sum (gap -> the zero row / column n)"""
    out = []
    for k0 in range(0, idx.shape[0], chunk):
        ix = idx[k0:k0 + chunk]
        quad = mJz[ix[:, :, None], ix[:, None, :]].sum(dim=(1, 2))
        out.append(0.5 * (quad - 2.0 * g[ix].sum(dim=1) + c0))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C", choices=sorted(CONFIGS))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-repeats", type=int, default=10)
    ap.add_argument("--pseudocount", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "energy_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 10, "at least 10 timed repeats"

    import gaussdca.jl_amd as gd
    from gaussdca.jl_amd import devops
    from gaussdca.jl_amd.synth import synth_family

    c = CONFIGS[args.config]
    N, M, q, theta, pc = c["N"], c["M"], 21, c["theta"], args.pseudocount
    s, n, K = q - 1, N * (q - 1), M
    stream = torch.cuda.current_stream()
    with step_limit(60, "contexts"):
        ctx = gd.Context(0, stream=stream.cuda_stream)  # the torch stream: its events time the library's kernels
        torch.cuda.synchronize()
    Zo = synth_family(N, M, q, c["seed"])  # (M, N)
    with step_limit(60, "upload"):
        dZ = torch.from_numpy(Zo).cuda()
        dS = torch.empty(N * N, dtype=torch.float64, device="cuda")
        dE = torch.empty(K, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
    res = dict(config=args.config, N=N, M=M, K=K, q=q, n=n, theta=theta, pseudocount=pc, repeats=args.repeats)

    # ---- a plain gdca_run and the fused energies run, same family, same process
    with step_limit(120, "gdca_run"):
        sts = []
        for i in range(args.warmup + args.repeats):
            st = ctx.run_dev(dZ.data_ptr(), N, M, q, pc, theta, 0, dS.data_ptr())
            if i >= args.warmup:
                sts.append(st)
        res["run_ms_total"] = statistics.median(x["ms_total"] for x in sts)
        res["run_ms_score"] = statistics.median(x["ms_score"] for x in sts)
    with step_limit(180, "gdca_run_energies"):
        sts = []
        for i in range(args.warmup + args.repeats):
            st = ctx.run_energies_dev(dZ.data_ptr(), N, M, q, pc, theta, None, 0, dE.data_ptr())
            if i >= args.warmup:
                sts.append(st)
        res["fused_ms_total"] = statistics.median(x["ms_total"] for x in sts)
        res["fused_ms_score"] = statistics.median(x["ms_score"] for x in sts)
        res["fused_ms_score_all"] = [x["ms_score"] for x in sts]
        res["fused_ms_inverse"] = statistics.median(x["ms_inverse"] for x in sts)
        E_fused = dE.clone()
        torch.cuda.synchronize()

    # ---- the operator on a resident mJ (built by the library's own device operators)
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
    with step_limit(180, "gdca_energies_dev"):
        ms = timed(lambda: ctx.energies_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dZ.data_ptr(), K, dE.data_ptr()), args.warmup, args.repeats)
        res["operator_ms"] = statistics.median(ms)
        res["operator_ms_all"] = ms
        E_op = dE.clone()
        torch.cuda.synchronize()
        res["fused_vs_operator_max_rel"] = float(((E_fused - E_op).abs() / E_op.abs()).max())

    # ---- rooflines of the energy stage
    tri_bytes = 8.0 * n * (n + s) / 2 + float(N) * K        # one pass over the lower block triangle of mJ, plus X
    gathers = float(K) * (N * (N + 1) / 2 + N)               # ds_read_b64 lane reads: the pairs i >= j, and g
    res["compulsory_bytes"] = tri_bytes
    res["hbm_ms_at_fn_rate"] = [tri_bytes / (f * PEAK_HBM) * 1e3 for f in FN_HBM_FRACTION]
    res["lds_gathers"] = gathers
    res["lds_ms_conflict_free"] = gathers / (CUS * GHZ * 1e9 * LDS_B64_PER_CLK) * 1e3
    # what the chosen tiling really moves: every workgroup (site block I, 2048 or 512 sequences) loads the tiles (I, 0 .. I) itself, so
    # the triangle is read once per sequence chunk (from L2 / the Infinity Cache where neighbours share it, from HBM otherwise)
    nI = (N + 3) // 4
    per = 2048 if -(-K // 2048) * nI >= 2 * CUS else 512
    res["tiling_triangle_passes"] = -(-K // per)
    res["tiling_bytes"] = res["tiling_triangle_passes"] * 8.0 * n * (n + s) / 2 + float(N) * K + 4.0 * nI * K * (nI + 1) / 2
    res["tiling_ms_at_fn_rate"] = [res["tiling_bytes"] / (f * PEAK_HBM) * 1e3 for f in FN_HBM_FRACTION]
    roof = max(min(res["hbm_ms_at_fn_rate"]), res["lds_ms_conflict_free"])
    res["roofline_ms"] = roof
    res["roofline_fraction_operator"] = roof / res["operator_ms"]
    res["roofline_fraction_fused"] = roof / res["fused_ms_score"]

    # ---- the same energies by torch on the same GPU
    with step_limit(600, "torch formulation"):
        mJz = torch.zeros((n + 1, n + 1), dtype=torch.float64, device="cuda")
        mJz[:n, :n] = dmJ.view(n, n)
        del dmJ
        Zl = dZ.long()
        idx = torch.where(Zl < q, torch.arange(N, device="cuda")[None, :] * s + Zl - 1, torch.full_like(Zl, n))  # (K, N)
        gz = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
        gz[:n] = mJz[:n, :n] @ dPi
        c0 = (dPi * gz[:n]).sum()
        chunk = max(1, (1 << 30) // (8 * N * N))  # 1 GB of gathered entries at a time
        holder = {}

        def run_torch():
            holder["E"] = torch_energies(mJz, gz, c0, idx, chunk)

        ms = timed(run_torch, args.warmup, args.torch_repeats)
        res["torch_ms"] = statistics.median(ms)
        res["torch_ms_all"] = ms
        res["torch_chunk"] = chunk
        res["torch_vs_operator_max_rel"] = float(((holder["E"] - E_op).abs() / E_op.abs()).max())
    res["speedup_vs_torch_operator"] = res["torch_ms"] / res["operator_ms"]
    res["speedup_vs_torch_fused_stage"] = res["torch_ms"] / res["fused_ms_score"]
    res["energies_on_top_of_a_fit_ms"] = res["fused_ms_total"] - res["run_ms_total"]
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
