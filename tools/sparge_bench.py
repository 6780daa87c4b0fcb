#!/usr/bin/env python3
"""The block-map predictor (sage_block_pool_sim, sage_block_select) measured in ONE process with alternating windows
(HIP events around `--launches` launches each), on clustered synthetic inputs (tests/sparge_util.py's generator at scale:
per 128-row q-block / 64-row key block a centre ~ N(0, 4 I), tokens = centre + N(0, I), every 4th q-block and every 5th key
block pure noise, K shifted by +3 on every channel).

  1. block_pool_sim on K beside sage_k_mean on the same K (k_mean_partial reads the same bytes): time and GB/s from the
     bytes of the shape.  `--mode kernels` only launches those kernels a few times, for `rocprofv3 --kernel-trace --stats`.
  2. the predictor (pool Q + pool K + select) as a share of the dense sageattn call and of the resulting sparse call.
  3. at cdfthreshd 0.9 / 0.95 / 0.98: density of the predicted map, end-to-end sageattn_sparge against dense sageattn, and
     calc_diff (1 - 2<x,y>/(|x|^2+|y|^2)) of its output against dense sageattn's.  With `--pvthreshd T` two more columns:
     the share of the kept wave-tiles whose softmax and P.V the second stage skipped at that threshold (from the counters of
     return_skipped) and calc_diff of that output against dense.
  4. the selection launch alone (sage_block_select on ready statistics) under both rules, in alternating windows; with
     `--parent-lib` also sage_block_select_cdf of that library (a build of the parent commit) in the same rotation, with the
     spread of its repeated windows as the margin and a bit-for-bit comparison of the lists.
  5. at each topk of `--topks`: density, list lengths (overall, and per head over its self-similar q-blocks), the sparse
     call's time beside the CDF run of the nearest density, end to end and calc_diff as in 3.
SYNTHETIC data: the densities and errors say nothing about a real model.

usage: sparge_bench.py [--launches 300] [--shapes c3,wan] [--pv fp16] [--mode all|kernels] [--topks 0.125,0.25,0.5]
                       [--pvthreshd T] [--parent-lib parent.so] [--commit HASH] [--out table.md]"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import sageattention_amd as sa  # noqa: E402
from sageattention_amd import _lib as L, core, quant  # noqa: E402

SHAPES = {"c3": (4, 32, 8192, 128), "wan": (1, 40, 32760, 128), "small": (2, 4, 2048, 128)}
ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=300)
ap.add_argument("--shapes", default="c3,wan")
ap.add_argument("--pv", default="fp16")
ap.add_argument("--mode", default="all", choices=("all", "kernels"))
ap.add_argument("--simthreshd1", type=float, default=0.6)
ap.add_argument("--cdfs", default="0.9,0.95,0.98")
ap.add_argument("--topks", default="0.125,0.25,0.5")
ap.add_argument("--pvthreshd", type=float, default=None, help="second stage: skip negligible wave-tiles at this threshold")
ap.add_argument("--parent-lib", default="", help="a build of the parent commit: its sage_block_select_cdf is the yardstick")
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()
lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


def clustered(B, H, n, D, blk, noise_every, offset, gen):
    nb = (n + blk - 1) // blk
    c = torch.randn(B, H, nb, 1, D, generator=gen, device="cuda") * 2.0
    noisy = (torch.arange(nb, device="cuda") % noise_every == noise_every - 1).view(1, 1, nb, 1, 1)
    c = torch.where(noisy, torch.zeros_like(c), c)
    x = c + torch.randn(B, H, nb, blk, D, generator=gen, device="cuda")
    return (x.reshape(B, H, nb * blk, D)[:, :, :n] + offset).half().contiguous()


def window(fn, n):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n  # ms per call


def calc_diff(x, y):
    x, y = x.double(), y.double()
    return float(1 - 2 * (x * y).sum() / (x * x + y * y).sum())


def spread(ts):
    return f"median {statistics.median(ts):.4f} ms, min {min(ts):.4f}, max {max(ts):.4f}"


def load_parent(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    fn = lib.sage_block_select_cdf
    fn.restype, fn.argtypes = L.SIGNATURES["sage_block_select_cdf"]
    return lib


def lengths_per_head(bmap, selfsim):
    """list lengths of the self-similar q-blocks of every (b, h): (least per-head min, greatest per-head max, greatest
    per-head max - min, heads whose lengths are all equal, heads)"""
    cnt = bmap.sum(-1).float()
    lo = torch.where(selfsim, cnt, torch.full_like(cnt, float("inf"))).amin(-1)
    hi = torch.where(selfsim, cnt, torch.full_like(cnt, float("-inf"))).amax(-1)
    has = selfsim.any(-1)
    lo, hi = lo[has], hi[has]
    return int(lo.min()), int(hi.max()), int((hi - lo).max()), int((hi == lo).sum()), int(has.sum())


parent = load_parent(a.parent_lib) if a.parent_lib else None
emit("# Block-map predictor: times on MI355X")
emit()
emit(f"commit {a.commit or 'unknown'}; tools/sparge_bench.py, {a.launches} calls per window, HIP events, one process, windows")
emit(f"alternating.  fp16, per-thread scales, {a.pv.upper()} PV, simthreshd1 = {a.simthreshd1}.  Clustered SYNTHETIC inputs: densities and")
emit("errors below describe this generator, not a model.")
for sname in a.shapes.split(","):
    B, H, N, D = SHAPES[sname]
    gen = torch.Generator(device="cuda").manual_seed(N + D)
    q = clustered(B, H, N, D, 128, 4, 0.0, gen)
    k = clustered(B, H, N, D, 64, 5, 3.0, gen)
    v = torch.randn(B, H, N, D, generator=gen, device="cuda").half()
    km = quant.k_mean(k)
    nbytes = q.numel() * 2

    def pool_k():
        quant.block_pool_sim(k, 64, mean=km)

    def pool_q():
        quant.block_pool_sim(q, 128)

    def kmean():
        quant.k_mean(k)

    def predict(cdf=0.98, topk=None):
        return core._sparge_predict(q, k, km, "HND", D ** -0.5, False, (a.simthreshd1, cdf, topk, 0, 0))[0]

    if a.mode == "kernels":
        for _ in range(20):
            pool_k(); pool_q(); kmean(); predict(); predict(topk=0.25)
        torch.cuda.synchronize()
        continue
    emit()
    emit(f"## {sname} (B, H, N, D) = {(B, H, N, D)}: {nbytes / 1e6:.0f} MB per tensor")
    emit()
    emit("| call (host-timed, allocations included) | repeats | ms | GB/s of the tensor's bytes |")
    emit("|---|---|---|---|")
    rows = {"block_pool_sim(k - km, 64)": pool_k, "sage_k_mean(k) (partial + final)": kmean, "block_pool_sim(q, 128)": pool_q}
    ts = {n: [] for n in rows}
    for _ in range(3):
        for n, fn in rows.items():
            ts[n].append(window(fn, a.launches))
    for n in rows:
        med = statistics.median(ts[n])
        emit(f"| {n} | {spread(ts[n])} | {med:.4f} | {nbytes / med / 1e6:.0f} |")
    emit()
    emit("| cdfthreshd | density | tiles per q-block min / mean / max | predictor ms | dense sageattn ms | sparse call ms | predictor / dense | "
         "predictor / sparse | sageattn_sparge ms | speed-up over dense | calc_diff vs dense |"
         + (f" pvthreshd {a.pvthreshd:g}: skipped share of kept wave-tiles | ... calc_diff vs dense |" if a.pvthreshd else ""))
    emit("|---|---|---|---|---|---|---|---|---|---|---|" + ("---|---|" if a.pvthreshd else ""))
    dense_fn = sa.sageattn_qk_int8_pv_fp16_cuda if a.pv == "fp16" else sa.sageattn_qk_int8_pv_fp8_cuda
    o_dense = dense_fn(q, k, v)
    dense_all, cdf_runs = [], []
    for cdf in (float(x) for x in a.cdfs.split(",")):
        plan, bmap = sa.sparge_plan(q, k, simthreshd1=a.simthreshd1, cdfthreshd=cdf, km=km, return_map=True)
        cnt = bmap.sum(-1).float()
        dens = float(bmap.float().mean())
        t_p = window(lambda: predict(cdf), a.launches)
        t_d = window(lambda: dense_fn(q, k, v), a.launches)
        t_s = window(lambda: sa.sageattn_block_sparse(q, k, v, plan, pv=a.pv), a.launches)
        t_e = window(lambda: sa.sageattn_sparge(q, k, v, simthreshd1=a.simthreshd1, cdfthreshd=cdf, pv=a.pv), a.launches)
        dense_all.append(t_d)
        cdf_runs.append((cdf, dens, t_s))
        o = sa.sageattn_sparge(q, k, v, simthreshd1=a.simthreshd1, cdfthreshd=cdf, pv=a.pv)
        extra = ""
        if a.pvthreshd:
            o_pv, skipped = sa.sageattn_sparge(q, k, v, simthreshd1=a.simthreshd1, cdfthreshd=cdf, pv=a.pv,
                                               pvthreshd=a.pvthreshd, return_skipped=True)
            extra = f" {float(skipped.sum()) / (4.0 * float(bmap.sum())):.3f} | {calc_diff(o_pv, o_dense):.3e} |"
        emit(f"| {cdf} | {dens:.3f} | {int(cnt.min())} / {float(cnt.mean()):.1f} / {int(cnt.max())} | {t_p:.4f} | {t_d:.4f} | {t_s:.4f} | "
             f"{t_p / t_d:.4f} | {t_p / t_s:.4f} | {t_e:.4f} | {t_d / t_e:.2f} | {calc_diff(o, o_dense):.3e} |" + extra)
    emit()
    emit(f"dense sageattn, {len(dense_all)} repeated windows: {spread(dense_all)}")

    # ---- the selection launch alone, on ready statistics -----------------------------------------------------------------
    pq, sq = quant.block_pool_sim(q, 128)
    pk, sk = quant.block_pool_sim(k, 64, mean=km)
    thr = torch.full((H,), a.simthreshd1, dtype=torch.float32, device="cuda")
    selfsim = sq > a.simthreshd1
    lib = L.lib()
    nints = lib.sage_block_sparse_workspace_bytes(B, H, N, N) // 4
    stats = (pq.data_ptr(), sq.data_ptr(), pk.data_ptr(), sk.data_ptr(), B, H, H, N, N, D, D ** -0.5, thr.data_ptr())
    stream = L.stream_ptr(q.device)
    topks = [float(x) for x in a.topks.split(",")]
    pars = {x: torch.full((H,), x, dtype=torch.float32, device="cuda") for x in [0.98] + topks}

    def select_call(which, fn, rule, par):
        out = torch.zeros(nints, dtype=torch.int32, device="cuda")
        args = stats + ((par.data_ptr(),) if rule is None else (rule, par.data_ptr(), 0, 0)) + (out.data_ptr(), nints * 4, None, stream)

        def run():
            L.check(fn(*args), which)
        return run, out

    sel = {}
    if parent is not None:
        sel["parent commit: sage_block_select_cdf, cdfthreshd 0.98"] = select_call("parent", parent.sage_block_select_cdf, None, pars[0.98])
    sel["sage_block_select_cdf, cdfthreshd 0.98"] = select_call("cdf", lib.sage_block_select_cdf, None, pars[0.98])
    sel["sage_block_select, CDF, cdfthreshd 0.98"] = select_call("select cdf", lib.sage_block_select, L.SELECT_CDF, pars[0.98])
    for tk in topks:
        sel[f"sage_block_select, TOPK, topk {tk}"] = select_call("select topk", lib.sage_block_select, L.SELECT_TOPK, pars[tk])
    ts = {n: [] for n in sel}
    for _ in range(5):
        for n, (run, _) in sel.items():
            ts[n].append(window(run, 4 * a.launches))  # a short kernel: longer windows
    emit()
    emit(f"| selection launch alone (ready statistics, no map), 5 alternating windows of {4 * a.launches} launches | repeats | median us | lists |")
    emit("|---|---|---|---|")
    first = next(iter(sel.values()))[1]
    for n, (_, out) in sel.items():
        same = "-" if "TOPK" in n else ("reference" if out is first else f"identical: {torch.equal(out, first)}")
        emit(f"| {n} | {spread(ts[n])} | {statistics.median(ts[n]) * 1e3:.1f} | {same} |")

    # ---- the TOPK rule -------------------------------------------------------------------------------------------------------
    emit()
    emit("| rule | density | tiles per q-block min / mean / max | per head, self-similar q-blocks: least min / greatest max / greatest "
         "max - min / heads of one length | predictor ms | sparse call ms | nearest CDF run: cdfthreshd, density, sparse call ms | "
         "sageattn_sparge ms | speed-up over dense | calc_diff vs dense |")
    emit("|---|---|---|---|---|---|---|---|---|---|")
    t_dense = statistics.median(dense_all)
    for cdf, dens, t_s in cdf_runs:
        _, bmap = sa.sparge_plan(q, k, simthreshd1=a.simthreshd1, cdfthreshd=cdf, km=km, return_map=True)
        cnt = bmap.sum(-1).float()
        lo, hi, rng, eq, nh = lengths_per_head(bmap, selfsim)
        emit(f"| cdfthreshd {cdf} | {dens:.3f} | {int(cnt.min())} / {float(cnt.mean()):.1f} / {int(cnt.max())} | "
             f"{lo} / {hi} / {rng} / {eq} of {nh} | see above | {t_s:.4f} | - | see above | - | - |")
    for tk in topks:
        plan, bmap = sa.sparge_plan(q, k, simthreshd1=a.simthreshd1, topk=tk, km=km, return_map=True)
        cnt = bmap.sum(-1).float()
        dens = float(bmap.float().mean())
        lo, hi, rng, eq, nh = lengths_per_head(bmap, selfsim)
        t_p = window(lambda: predict(topk=tk), a.launches)
        t_s = window(lambda: sa.sageattn_block_sparse(q, k, v, plan, pv=a.pv), a.launches)
        t_e = window(lambda: sa.sageattn_sparge(q, k, v, simthreshd1=a.simthreshd1, topk=tk, pv=a.pv), a.launches)
        o = sa.sageattn_sparge(q, k, v, simthreshd1=a.simthreshd1, topk=tk, pv=a.pv)
        near = min(cdf_runs, key=lambda r: abs(r[1] - dens)) if cdf_runs else None
        near_s = f"{near[0]}, {near[1]:.3f}, {near[2]:.4f}" if near else "-"
        emit(f"| topk {tk} | {dens:.3f} | {int(cnt.min())} / {float(cnt.mean()):.1f} / {int(cnt.max())} | "
             f"{lo} / {hi} / {rng} / {eq} of {nh} | {t_p:.4f} | {t_s:.4f} | {near_s} | {t_e:.4f} | {t_dense / t_e:.2f} | "
             f"{calc_diff(o, o_dense):.3e} |")
    del pq, sq, pk, sk
    del q, k, v, o_dense
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
