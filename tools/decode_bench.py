#!/usr/bin/env python3
"""``sageattn_decode_paged`` (one wave per split) against ``sageattn_splitkv_paged(causal=True)`` on the same paged cache, in
ONE process with alternating windows as tools/splitkv_bench.py does.  What is timed is a whole decode step, {append of the
step's tile; attention}, captured into a HIP graph and replayed, so the host is out of the picture; a window is a warm-up and
then HIP events around enough replays to last about ``--window-ms``.  A time is the median over ``--repeats`` rounds, a ratio
the median of the per-round ratios with their least and greatest value.  The yardstick is timed twice per rotation ("again"):
its spread against itself is what a difference is judged by.  Variants per shape and P.V mode:

  decode, S = decode_num_splits      yardstick, S = splitkv_num_splits (its own choice), twice      yardstick, S of the decode call

and a sweep of the decode step over S = 1..16.  The attention and merge kernel times come from torch.profiler traces of the same
graphs' replays, in passes of their own behind the timed windows: three traces of 20 replays per variant, the median with the
least and greatest beside it, "yardstick again" from its own graph; effective bytes per second are the K + V bytes of the cache (INT8 K, FP16 or FP8 V, every sequence at full length)
over the attention kernel's time.  Shapes (B, Hq, T, N, D), folded by g = 4 (Hk = Hq / 4):

  (8, 32, 1, 8192, 128)     a decode step                         (64, 32, 1, 8192, 128)   ... of a large batch
  (1, 32, 1, 65536, 128)    one long sequence                     (8, 32, 4, 8192, 128)    4 speculative tokens: q [8, 8, 16, 128]

``--pv fp4`` measures ``sageattn_decode_paged_v4`` on a ``SagePagedKVCacheV4`` instead: the yardstick is
``sageattn_splitkv_paged_v4(causal=True)`` on the same cache, and a second one, "decode, FP8 cache", is ``sageattn_decode_paged``
on a ``SagePagedKVCache(pv="fp8")`` over the same pools (profiles/decode_fp4.md).

There is no pass / fail time.  usage: decode_bench.py [--repeats 5] [--window-ms 100] [--pv fp16,fp8,fp4] [--shapes 0,1,2,3] [--out F]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import sageattention_amd as sa  # noqa: E402
from sageattention_amd import core  # noqa: E402

SHAPES = [(8, 32, 1, 8192, 128), (64, 32, 1, 8192, 128), (1, 32, 1, 65536, 128), (8, 32, 4, 8192, 128)]
G, PAGE = 4, 256

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window-ms", type=float, default=100.0)
ap.add_argument("--pv", default="fp16,fp8")
ap.add_argument("--shapes", default="0,1,2,3")
ap.add_argument("--out", default="")
a = ap.parse_args()
lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


def events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3  # us per call


def graph_of(step):
    step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    return g.replay


def rounds(variants, repeats):
    calls = {}
    for name, fn in variants.items():
        for _ in range(3):
            fn()
        calls[name] = max(5, int(a.window_ms * 1e3 / max(events(fn, 5), 1.0)))
    out = {name: [] for name in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            for _ in range(3):
                fn()
            out[name].append(events(fn, calls[name]))
    return out


def kernel_us(replay, attn_name, calls=20, passes=3):
    """device time (us) of the attention and the merge kernel inside the replayed graph, from torch.profiler traces in a pass of
    their own: ``passes`` traces of ``calls`` replays each -> (median attn, least, greatest, median merge).  NaN where the
    trace lists no such kernel."""
    from torch.profiler import ProfilerActivity, profile
    attn, merge = [], []
    for _ in range(passes):
        replay()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                replay()
            torch.cuda.synchronize()
        got = {}
        for it in prof.key_averages():
            tot = getattr(it, "self_device_time_total", 0.0) or getattr(it, "self_cuda_time_total", 0.0) or 0.0
            for key in (attn_name, "splitkv_merge_kernel"):
                if key in it.key and tot:
                    t, n = got.get(key, (0.0, 0))
                    got[key] = (t + tot, n + it.count)
        at, mg = (got[k][0] / got[k][1] if k in got else float("nan") for k in (attn_name, "splitkv_merge_kernel"))
        attn.append(at); merge.append(mg)
    return statistics.median(attn), min(attn), max(attn), statistics.median(merge)


def fmt_ratio(ts, base):
    r = [x / y for x, y in zip(ts, base)]
    return f"{statistics.median(r):.3f} ({min(r):.3f} .. {max(r):.3f})"


def setup(B, Hq, T, N, D, pv):
    Hk, P = Hq // G, B * N // PAGE
    gen = torch.Generator(device="cuda").manual_seed(B + N)
    k = torch.randn(P, Hk, PAGE, D, generator=gen, device="cuda", dtype=torch.float16)
    v = torch.randn(P, Hk, PAGE, D, generator=gen, device="cuda", dtype=torch.float16)
    table = torch.randperm(P, generator=gen, device="cuda").to(torch.int32).view(B, N // PAGE)
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    cache = sa.SagePagedKVCacheV4.prepare(k, v, table, lens) if pv == "fp4" else sa.SagePagedKVCache.prepare(k, v, table, lens, pv=pv)
    cache8 = sa.SagePagedKVCache.prepare(k, v, table, lens, pv="fp8") if pv == "fp4" else None  # the second yardstick's cache
    q = torch.randn(B, Hk, T * G, D, generator=gen, device="cuda", dtype=torch.float16)
    return cache, cache8, table, lens, q


def main():
    assert torch.cuda.is_available(), "decode_bench.py measures on the GPU: there is no fallback"
    emit(f"device: {torch.cuda.get_device_name(0)}; windows of {a.window_ms:.0f} ms, {a.repeats} rounds; pages of {PAGE} keys")
    for si in (int(s) for s in a.shapes.split(",")):
        B, Hq, T, N, D = SHAPES[si]
        for pv in a.pv.split(","):
            cache, cache8, table, lens, q = setup(B, Hq, T, N, D, pv)
            Hk = Hq // G
            fp4 = pv == "fp4"
            # (FP4: half a byte per element of V and 2 * D scale bytes per 64 keys)
            kv_bytes = B * Hk * N * (D * 3 // 2 + D // 32) if fp4 else B * Hk * N * D * (1 + (1 if pv == "fp8" else 2))
            f_dec = sa.sageattn_decode_paged_v4 if fp4 else sa.sageattn_decode_paged
            f_yard = sa.sageattn_splitkv_paged_v4 if fp4 else sa.sageattn_splitkv_paged
            k_dec = "attn_i8_decode_paged_v4_kernel" if fp4 else "attn_i8_decode_paged_kernel"
            k_yard = "attn_i8_splitkv_causal_paged_v4_kernel" if fp4 else "attn_i8_splitkv_causal_paged_kernel"
            s_dec, s_yard = sa.decode_num_splits(B, Hk, N), core.splitkv_num_splits(B, Hk, T * G, N)

            def dec(S):
                return lambda: f_dec(q, cache, table, lens, num_splits=S, q_fold=G, return_lse=True)

            def yard(S):
                return lambda: f_yard(q, cache, table, lens, num_splits=S, causal=True, q_fold=G, return_lse=True)

            def step(attn):
                def run():
                    cache.append(table, lens, lens, 1)
                    attn()
                return graph_of(run)

            same = all(torch.equal(x, y) for x, y in zip(dec(s_dec)(), yard(s_dec)()))
            emit()
            emit(f"## ({B}, {Hq}, {T}, {N}, {D}) folded by {G}, {pv.upper()} P.V: K + V = {kv_bytes / 1e6:.1f} MB; decode S = {s_dec}, "
                 f"yardstick S = {s_yard}; bits equal at S = {s_dec}: {same}")
            variants = {"decode": step(dec(s_dec)), "yardstick": step(yard(s_yard)), "yardstick again": step(yard(s_yard)),
                        "yardstick, equal S": step(yard(s_dec))}
            if fp4:  # the FP8 cache's own append and its one-wave kernel, over the same pools
                def step8():
                    cache8.append(table, lens, lens, 1)
                    sa.sageattn_decode_paged(q, cache8, table, lens, num_splits=s_dec, q_fold=G, return_lse=True)
                variants["decode, FP8 cache"] = graph_of(step8)
            ts = rounds(variants, a.repeats)
            emit("| variant | step us (median) | / yardstick | attention us (least .. greatest of 3 traces) | merge us | K + V TB/s |")
            emit("|---|---|---|---|---|---|")
            for name, t in ts.items():  # every variant's kernels out of its OWN graph's replays
                at, lo, hi, mg = kernel_us(variants[name], k_dec if name == "decode" else "attn_i8_decode_paged_kernel"
                                           if name == "decode, FP8 cache" else k_yard)
                emit(f"| {name} | {statistics.median(t):.1f} | {fmt_ratio(t, ts['yardstick'])} | {at:.1f} ({lo:.1f} .. {hi:.1f}) | "
                     f"{mg:.1f} | {kv_bytes / at / 1e6:.2f} |")
            sweep = {f"S={S}": step(dec(S)) for S in range(1, 17)}
            st = rounds(sweep, max(2, a.repeats // 2))
            emit("decode step us over S = 1..16: " + " ".join(f"{statistics.median(st[f'S={S}']):.1f}" for S in range(1, 17)))
            del cache, cache8, table, lens, q
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
