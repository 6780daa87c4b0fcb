#!/usr/bin/env python3
"""``sageattn_decode_paged_window`` (one wave per split; one launch at S = 1) against ``sageattn_splitkv_paged_window`` on the
same paged cache, in ONE process with alternating windows as tools/decode_bench.py does.  What is timed is a whole decode step,
{append of the step's tile; attention}, captured into a HIP graph and replayed; a window is a warm-up and then HIP events around
enough replays to last about ``--window-ms``.  A time is the median over ``--repeats`` rounds, a ratio the median of the
per-round ratios with their least and greatest value.  The yardstick is timed twice per rotation ("again"): its spread against
itself is what a difference is judged by.  Variants per shape and P.V mode:

  decode window, S = its rule      decode window, S = 1 (one launch)      decode window, S = 2 (the two-launch path)
  yardstick, S = its own rule, twice      yardstick, S = 1

and a sweep of the decode step over S = 1..16, which judges the ``num_splits=None`` guess.  The two-launch path of the one-wave
kernel at S = 1 cannot be reached through the interface (the entry fuses iff S == 1): what the finish inside the launch saves
is read from the kernel times -- the yardstick's merge kernel at S = 1 against nothing -- and from S = 1 against S = 2.  Kernel
times come from torch.profiler traces of the same graphs' replays, in passes of their own: three traces of 20 replays, the median
with the least and greatest beside it.  Shapes (name, B, Hq, g, D, window, sinks), T = 1, 8192 keys per sequence:

  gpt-oss-like   Hq 64 / Hk 8 folded by 8, head_dim 64, window 128, sinks        B = 8 and 64
  Mistral-like   Hq 32 / Hk 8 folded by 4, head_dim 128, window 4096             B = 8 and 64
  full window    Hq 64 / Hk 8 folded by 8, head_dim 64, window 8192, sinks       B = 8

There is no pass / fail time.  usage: decode_window_bench.py [--repeats 5] [--window-ms 100] [--pv fp16,fp8] [--shapes 0,1,2,3,4]
[--out F]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import sageattention_amd as sa  # noqa: E402
from sageattention_amd import core, decode_window, window as W  # noqa: E402

N, PAGE = 8192, 256
SHAPES = [("gpt-oss-like", 8, 64, 8, 64, 128, True), ("gpt-oss-like", 64, 64, 8, 64, 128, True),
          ("Mistral-like", 8, 32, 4, 128, 4096, False), ("Mistral-like", 64, 32, 4, 128, 4096, False),
          ("full window", 8, 64, 8, 64, 8192, True)]

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window-ms", type=float, default=100.0)
ap.add_argument("--pv", default="fp16,fp8")
ap.add_argument("--shapes", default="0,1,2,3,4")
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


def kernel_us(replay, calls=20, passes=3):
    """device time (us) of the attention and the merge kernel inside the replayed graph -> (median attn, least, greatest, median
    merge); the merge is NaN where the trace lists none (the one-launch path)"""
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
            for key in ("window_kernel", "window_merge_kernel"):
                if key in it.key and tot:
                    t, n = got.get(key, (0.0, 0))
                    got[key] = (t + tot, n + it.count)
        at, mg = (got[k][0] / got[k][1] if k in got else float("nan") for k in ("window_kernel", "window_merge_kernel"))
        attn.append(at); merge.append(mg)
    return statistics.median(attn), min(attn), max(attn), statistics.median(merge)


def fmt_ratio(ts, base):
    r = [x / y for x, y in zip(ts, base)]
    return f"{statistics.median(r):.3f} ({min(r):.3f} .. {max(r):.3f})"


def main():
    assert torch.cuda.is_available(), "decode_window_bench.py measures on the GPU: there is no fallback"
    emit(f"device: {torch.cuda.get_device_name(0)}; windows of {a.window_ms:.0f} ms, {a.repeats} rounds; {N} keys per sequence, "
         f"pages of {PAGE}")
    for si in (int(s) for s in a.shapes.split(",")):
        name, B, Hq, G, D, window, with_sinks = SHAPES[si]
        Hk, P = Hq // G, B * N // PAGE
        for pv in a.pv.split(","):
            gen = torch.Generator(device="cuda").manual_seed(B + N)
            k = torch.randn(P, Hk, PAGE, D, generator=gen, device="cuda", dtype=torch.float16)
            v = torch.randn(P, Hk, PAGE, D, generator=gen, device="cuda", dtype=torch.float16)
            table = torch.randperm(P, generator=gen, device="cuda").to(torch.int32).view(B, N // PAGE)
            lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
            cache = sa.SagePagedKVCache.prepare(k, v, table, lens, pv=pv)
            q = torch.randn(B, Hk, G, D, generator=gen, device="cuda", dtype=torch.float16)
            sinks = torch.randn(Hq, generator=gen, device="cuda") if with_sinks else None
            s_dec = decode_window._num_splits(B, Hk, N, window, G, G)
            s_yard = core.splitkv_num_splits(B, Hk, G, W._windowed_keys(table, cache, window, G))

            def dec(S):
                return lambda: sa.sageattn_decode_paged_window(q, cache, table, lens, window, num_splits=S, q_fold=G, sinks=sinks,
                                                               return_lse=True)

            def yard(S):
                return lambda: sa.sageattn_splitkv_paged_window(q, cache, table, lens, window, num_splits=S, q_fold=G,
                                                                sinks=sinks, return_lse=True)

            def step(attn):
                def run():
                    cache.append(table, lens, lens, 1)
                    attn()
                return graph_of(run)

            same = all(torch.equal(x, y) for S in {1, s_dec} for x, y in zip(dec(S)(), yard(S)()))
            emit()
            emit(f"## {name}: B = {B}, Hq {Hq} / Hk {Hk} folded by {G}, head_dim {D}, window {window}, sinks: {with_sinks}, "
                 f"{pv.upper()} P.V; decode S = {s_dec}, yardstick S = {s_yard}; bits equal at S = 1 and {s_dec}: {same}")
            variants = {"decode window": step(dec(s_dec)), "decode window, S = 1 (one launch)": step(dec(1)),
                        "decode window, S = 2 (two launches)": step(dec(2)), "yardstick": step(yard(s_yard)),
                        "yardstick again": step(yard(s_yard)), "yardstick, S = 1": step(yard(1))}
            ts = rounds(variants, a.repeats)
            emit("| variant | step us (median) | / yardstick | attention us (least .. greatest of 3 traces) | merge us |")
            emit("|---|---|---|---|---|")
            for vn, t in ts.items():
                at, lo, hi, mg = kernel_us(variants[vn])
                emit(f"| {vn} | {statistics.median(t):.1f} | {fmt_ratio(t, ts['yardstick'])} | {at:.1f} ({lo:.1f} .. {hi:.1f}) | {mg:.1f} |")
            sweep = {f"S={S}": step(dec(S)) for S in range(1, 17)}
            st = rounds(sweep, max(2, a.repeats // 2))
            emit("decode window step us over S = 1..16: " + " ".join(f"{statistics.median(st[f'S={S}']):.1f}" for S in range(1, 17)))
            del cache, table, lens, q, k, v
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
