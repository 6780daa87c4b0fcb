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

With --pvthreshd T the tool measures the P.V skip instead (sage_attn_qk_int8_pv_{f16,f8}_blocksparse_pvskip) and writes
profiles/pvskip_sweep.md unless --out says otherwise:
  cost   the skip kernel at threshold 1e30 (it never skips) against the block-sparse kernel without the skip, random maps of
         density 1 and 1/4, windows alternating, `--repeats` windows each; the yardstick is the spread of the repeated
         windows of the kernel without the skip
  gain   all tiles kept, keys built so that about 1/4, 1/2 and 3/4 of the wave-tiles lie 30 below the row maximum
         (tests/pvskip_util.py's generator at these shapes), threshold T: time and the skipped share read from the
         counters, beside the same call without the skip

usage: blocksparse_bench.py [--launches 300] [--shapes c3,d64,wan,short] [--pv fp16,fp8] [--commit HASH] [--out table.md]
       blocksparse_bench.py --pvthreshd 16 [--shapes c3,d64] [--repeats 4] ..."""
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
ap.add_argument("--pvthreshd", type=float, default=None)
ap.add_argument("--repeats", type=int, default=4)
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


def write_out(default=""):
    out = a.out or default
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def pvskip_sweep():
    thr_v = a.pvthreshd
    emit("# P.V skip of block-sparse attention: kernel times on MI355X")
    emit()
    emit(f"commit {a.commit or 'unknown'}; tools/blocksparse_bench.py --pvthreshd {thr_v:g}, {a.launches} launches per window, HIP")
    emit(f"events, one process, the variants of a row alternating, {a.repeats} windows each (medians).  per-thread scales, fp16")
    emit("tensors, int8-Q entry points.  plain = sage_attn_qk_int8_pv_*_blocksparse, skip = its _pvskip twin with counters.")
    shapes = [x for x in a.shapes.split(",") if x in ("c3", "d64")] or ["c3", "d64"]
    for sname in shapes:
        B, H, N, D = SHAPES[sname]
        M = N
        nqb, ntk = (M + 127) // 128, (N + 63) // 64
        nbytes = lib.sage_block_sparse_workspace_bytes(B, H, M, N)
        lists = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
        skipped = torch.empty(B, H, nqb, 4, dtype=torch.int32, device="cuda")
        thr = torch.empty(H, dtype=torch.float32, device="cuda")
        o = torch.empty(B, H, N, D, dtype=torch.float16, device="cuda")
        tail = (None, None, B, H, H, M, N, D, 0, 3, 128, 32, D ** -0.5, 0)

        def operands(q, k, v):
            k8, ks, km = core._prep_k(k, "HND", "per_thread", True)
            q8, qs, _ = core._quant_q(q, km, "HND", "per_thread", D ** -0.5, 32, False, H, H)
            v8, vs, _ = sa.quant.per_channel_fp8(v, tensor_layout="HND", smooth_v=False)
            v8d = L.SageTensor(v8.data_ptr(), v8.stride(0), v8.stride(1), v8.stride(2))
            dq, dk, dv, do = (L.desc(t, "HND") for t in (q8, k8, v, o))
            keep = (q8, qs, k8, ks, v8, vs, v)
            return {"fp16": ((dq, dk, dv, 0, do, 0, qs.data_ptr(), ks.data_ptr()), "sage_attn_qk_int8_pv_f16_blocksparse"),
                    "fp8": ((dq, dk, v8d, do, 0, qs.data_ptr(), ks.data_ptr(), vs.data_ptr()),
                            "sage_attn_qk_int8_pv_f8_blocksparse")}, keep

        def compact(bm):
            bmv = bm.view(1, 1, nqb, ntk).expand(B, H, nqb, ntk)
            L.check(lib.sage_block_map_compact(bmv.data_ptr(), (ctypes.c_int64 * 4)(*bmv.stride()), B, H, M, N,
                                               lists.data_ptr(), nbytes, st), "compact")

        def pair(head, name):
            def plain():
                L.check(getattr(lib, name)(*head, *tail, lists.data_ptr(), nbytes, st), name)

            def skip():
                L.check(getattr(lib, name + "_pvskip")(*head, *tail, lists.data_ptr(), nbytes, thr.data_ptr(),
                                                       skipped.data_ptr(), st), name + "_pvskip")
            return plain, skip

        def alternate(plain, skip):
            tp, ts = [], []
            for _ in range(a.repeats):
                tp.append(window(plain, a.launches))
                ts.append(window(skip, a.launches))
            return tp, ts

        # ---- cost of the check: random data, the skip kernel never skips
        torch.manual_seed(0)
        q, k, v = (torch.randn(B, H, N, D, dtype=torch.float16, device="cuda") for _ in range(3))
        ops, keep = operands(q, k, v)
        thr.fill_(1e30)
        emit()
        emit(f"## {sname} (B, H, N, D) = {(B, H, N, D)}: cost of the check (threshold 1e30, nothing skipped)")
        emit()
        emit("| PV | density | t_plain ms (median) | plain spread % | t_skip ms (median) | t_skip / t_plain | difference vs spread |")
        emit("|---|---|---|---|---|---|---|")
        for pv in a.pv.split(","):
            for dens in (1.0, 0.25):
                bm = make_map("random", nqb, ntk, dens, seed=int(dens * 1000) + N).cuda()
                compact(bm)
                tp, ts = alternate(*pair(*ops[pv]))
                assert int(skipped.abs().sum()) == 0
                mp, ms = statistics.median(tp), statistics.median(ts)
                spread = 100 * (max(tp) - min(tp)) / mp
                diff = 100 * (ms - mp) / mp
                verdict = "inside" if abs(diff) <= spread else f"outside by {abs(diff) - spread:.2f} points"
                emit(f"| {pv} | {float(bm.float().mean()):.3f} | {mp:.4f} | {spread:.2f} | {ms:.4f} | {ms / mp:.4f} | "
                     f"{diff:+.2f} % ({verdict}) |")
        del q, k, ops, keep
        # ---- gain: every tile kept, a share of them 30 below the row maximum
        emit()
        emit(f"## {sname}: gain at pvthreshd = {thr_v:g} (all tiles kept; keys of the marked tiles 30 below the best)")
        emit()
        emit("| PV | tiles marked | skipped share (counters) | t_plain ms | t_skip ms | t_skip / t_plain |")
        emit("|---|---|---|---|---|---|")
        compact(torch.ones(nqb, ntk, dtype=torch.bool, device="cuda"))
        thr.fill_(thr_v)
        for share in (0.25, 0.5, 0.75):
            g = torch.Generator().manual_seed(int(share * 100) + N)
            low = torch.rand(ntk, generator=g) < share
            low[0] = False  # the first tile sets the maximum
            qq = 0.05 * torch.randn(B, H, N, D, generator=g)
            qq[..., 0] += 0.5 * D ** 0.5
            kk = 0.05 * torch.randn(B, H, N, D, generator=g)
            kk[..., 0] += (-60.0 * low.float()).repeat_interleave(64)[:N]
            ops, keep = operands(qq.half().cuda(), kk.half().cuda(), v)
            for pv in a.pv.split(","):
                tp, ts = alternate(*pair(*ops[pv]))
                got = float(skipped.sum()) / (B * H * nqb * 4 * ntk)
                mp, ms = statistics.median(tp), statistics.median(ts)
                emit(f"| {pv} | {float(low.float().mean()):.3f} | {got:.3f} | {mp:.4f} | {ms:.4f} | {ms / mp:.3f} |")
            del ops, keep
        del v, o, lists
        torch.cuda.empty_cache()
    write_out("profiles/pvskip_sweep.md")


if a.pvthreshd is not None:
    if not a.pvthreshd > 0:
        sys.exit("--pvthreshd must be > 0")
    pvskip_sweep()
    sys.exit(0)

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
write_out()
