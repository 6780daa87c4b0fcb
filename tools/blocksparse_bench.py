#!/usr/bin/env python3
"""Block-sparse attention against the dense 4-wave kernel and the masked operator, kernel level, in ONE process with
alternating windows (HIP events around `--launches` launches each).

For every shape x PV type x density x pattern:
  (a) dense   sage_attn_qk_int8_pv_{f16,f8}, geometry pinned to 4 waves (the geometry the sparse kernel always has);
              measured again in front of every sparse window: the spread of those repeats is the noise of the table
  (b) sparse  sage_attn_qk_int8_pv_{f16,f8}_blocksparse on the compacted lists
  (c) masked  sage_attn_qk_int8_pv_f16_masked on the map expanded to a bool [M,N] mask (FP16 PV only): what a caller had
              to use before
and the time of sage_block_map_compact.  The map is [1,1,ceil(M/128),ceil(N/64)], shared by batch and heads (a static
pattern), so that the expanded mask of (c) stays small enough to build.  Patterns: seeded random tiles, and a band of constant
width around the diagonal (both with the exact density printed, at least one tile per q-block).

usage: blocksparse_bench.py [--launches 300] [--shapes c3,d64,wan,short] [--pv fp16,fp8] [--commit HASH] [--out table.md]"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import sageattention_amd as sa  # noqa: E402
from sageattention_amd import _lib as L, core  # noqa: E402

SHAPES = {"c3": (4, 32, 8192, 128), "d64": (4, 32, 8192, 64), "wan": (1, 40, 32760, 128),
          "short": (4, 32, 1024, 128)}  # short: what the fixed costs of a sparse call (lists, the empty-row launch) weigh
ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=300)
ap.add_argument("--shapes", default="c3,d64,wan,short")
ap.add_argument("--pv", default="fp16,fp8")
ap.add_argument("--densities", default="1,0.5,0.25,0.125")
ap.add_argument("--patterns", default="random,band")
ap.add_argument("--no-masked", action="store_true")
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()
lib = L.lib()
st = torch.cuda.current_stream().cuda_stream
lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


def make_map(pattern, nqb, ntk, density, seed):
    want = max(1, round(density * ntk))
    bm = torch.zeros(nqb, ntk, dtype=torch.bool)
    if pattern == "band":  # `want` tiles around the diagonal, the window pushed inwards at the edges
        for i in range(nqb):
            lo = int(round((i + 0.5) * ntk / nqb - want / 2))
            lo = min(max(lo, 0), ntk - want)
            bm[i, lo:lo + want] = True
    else:
        g = torch.Generator().manual_seed(seed)
        bm = torch.rand(nqb, ntk, generator=g) < density
        if density >= 1:
            bm[:] = True
        empty = torch.nonzero(~bm.any(-1)).flatten()
        bm[empty, torch.randint(0, ntk, (empty.numel(),), generator=g)] = True
    return bm


def window(fn, n):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n  # ms per launch


emit("# Block-sparse attention: kernel times on MI355X")
emit()
emit(f"commit {a.commit or 'unknown'}; tools/blocksparse_bench.py, {a.launches} launches per window, HIP events, one process,")
emit("dense and sparse windows alternating.  per-thread scales, fp16 tensors, map shared by batch and heads.")
emit("efficiency = density * t_dense / t_sparse; dense = the 4-wave dense kernel; masked = sage_attn_qk_int8_pv_f16_masked")
emit("on the expanded bool mask.  `lists` = min / mean / max active tiles per q-block.")
for sname in a.shapes.split(","):
    B, H, N, D = SHAPES[sname]
    M = N
    nqb, ntk = (M + 127) // 128, (N + 63) // 64
    torch.manual_seed(0)
    q, k, v = (torch.randn(B, H, N, D, dtype=torch.float16, device="cuda") for _ in range(3))
    k8, ks, km = core._prep_k(k, "HND", "per_thread", True)
    q8, qs, _ = core._quant_q(q, km, "HND", "per_thread", D ** -0.5, 32, False, H, H)
    o = torch.empty_like(q)
    v8, vs, _ = sa.quant.per_channel_fp8(v, tensor_layout="HND", smooth_v=False)
    v8d = L.SageTensor(v8.data_ptr(), v8.stride(0), v8.stride(1), v8.stride(2))
    dq, dk, dv, do = (L.desc(t, "HND") for t in (q8, k8, v, o))
    tail = (None, None, B, H, H, M, N, D, 0, 3, 128, 32, D ** -0.5, 0)
    nbytes = lib.sage_block_sparse_workspace_bytes(B, H, M, N)
    lists = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
    for pv in a.pv.split(","):
        if pv == "fp16":
            head = (dq, dk, dv, 0, do, 0, qs.data_ptr(), ks.data_ptr())
            names = ("sage_attn_qk_int8_pv_f16", "sage_attn_qk_int8_pv_f16_blocksparse")
        else:
            head = (dq, dk, v8d, do, 0, qs.data_ptr(), ks.data_ptr(), vs.data_ptr())
            names = ("sage_attn_qk_int8_pv_f8", "sage_attn_qk_int8_pv_f8_blocksparse")

        def dense():
            L.check(getattr(lib, names[0])(*head, *tail, st), names[0])

        def sparse():
            L.check(getattr(lib, names[1])(*head, *tail, lists.data_ptr(), nbytes, st), names[1])

        lib.sage_set_tuning(0, 4)
        emit()
        emit(f"## {sname} (B, H, N, D) = {(B, H, N, D)}, {pv.upper()} PV")
        emit()
        emit("| pattern | density | lists | t_dense ms | t_sparse ms | t_sparse / t_dense | efficiency | t_masked ms | t_masked / t_sparse | compact us |")
        emit("|---|---|---|---|---|---|---|---|---|---|")
        dense_all = []
        for pattern in a.patterns.split(","):
            for dens in (float(x) for x in a.densities.split(",")):
                bm = make_map(pattern, nqb, ntk, dens, seed=int(dens * 1000) + N).cuda()
                cnt = bm.sum(-1).float()
                real = float(bm.float().mean())
                bmv = bm.view(1, 1, nqb, ntk).expand(B, H, nqb, ntk)
                strides = (ctypes.c_int64 * 4)(*bmv.stride())

                def compact():
                    L.check(lib.sage_block_map_compact(bmv.data_ptr(), strides, B, H, M, N, lists.data_ptr(), nbytes, st), "compact")

                t_c = window(compact, a.launches)
                t_d = window(dense, a.launches)
                t_s = window(sparse, a.launches)
                dense_all.append(t_d)
                t_m = float("nan")
                if pv == "fp16" and not a.no_masked:
                    mask = bm.repeat_interleave(128, 0)[:M].repeat_interleave(64, 1)[:, :N].contiguous()
                    ms = (ctypes.c_int64 * 4)(0, 0, N, 1)
                    margs = (dq, dk, dv, 0, do, 0, qs.data_ptr(), ks.data_ptr(), mask.data_ptr(), 1, ms, None, B, H, H, M, N, D, 3,
                             128, 32, D ** -0.5, 0, st)

                    def masked():
                        L.check(lib.sage_attn_qk_int8_pv_f16_masked(*margs), "masked")

                    lib.sage_set_tuning(0, 0)  # the masked operator in the geometry the library picks for it
                    t_m = window(masked, a.launches)
                    lib.sage_set_tuning(0, 4)
                    del mask
                emit(f"| {pattern} | {real:.3f} | {int(cnt.min())} / {float(cnt.mean()):.1f} / {int(cnt.max())} | {t_d:.4f} | {t_s:.4f} | "
                     f"{t_s / t_d:.3f} | {real * t_d / t_s:.3f} | {t_m:.4f} | {t_m / t_s:.2f} | {1e3 * t_c:.1f} |")
        lib.sage_set_tuning(0, 0)
        med = statistics.median(dense_all)
        emit()
        emit(f"dense 4-wave kernel, {len(dense_all)} repeated windows: median {med:.4f} ms, min {min(dense_all):.4f}, "
             f"max {max(dense_all):.4f} (spread {100 * (max(dense_all) - min(dense_all)) / med:.2f} % of the median)")
    del q, k, v, q8, k8, v8, o
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
