#!/usr/bin/env python3
"""Whole-call times of sliding-window attention on the paged cache against the existing operators -> profiles/window.md.

    python tools/window_bench.py [--out profiles/window.md] [--rotations 5]

Two shapes, every sequence at 8192 keys, Hq 32 / Hk 8 folded (g = 4), head_dim 128, page size 64, num_splits 4, both P.V types,
window 1024 and 4096:
  * decode: 8 sequences of one token, sageattn_splitkv_paged_window;
  * mixed: one prefill chunk of 2048 tokens plus 63 decode sequences, sageattn_splitkv_paged_ragged_window (plan made once).
Each against two calls of the existing causal paged / ragged operator: on the whole cache -- the yardstick, timed twice per
rotation; its two times give the spread a ratio is read against -- and restricted to the keys a window call walks (the table
row shifted to the window's first page, kv_lens = window + T_b - 1 rounded up to a page): the bound a window call can approach.
The restricted call computes something else for a chunk (its first tokens see the whole restricted range); it is a cost bound
only.  Times are HIP-event times of `iters` back-to-back calls, host side included, median over the rotations."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sageattention_amd as sa  # noqa: E402
from ragged_bench import D, G, HK, HQ, NKEYS, PAGE, fold, timed  # noqa: E402

CHUNK, S = 2048, 4
HEAD = """# Sliding-window attention on the paged cache: registers, accuracy and whole-call times

`python tools/window_bench.py` on one MI355X.  8192 keys per sequence, Hq 32 / Hk 8 folded (g = 4), head_dim 128, page size 64,
num_splits 4.  decode: 8 sequences of one token; mixed: 2048 + 63 x 1 tokens.  `whole` is the existing causal paged / ragged call
on the whole cache (timed twice: the spread), `restricted` the existing call on a table shifted to the window's first page with
kv_lens cut to the keys a window call walks (a cost bound, not the same result for a chunk).  HIP-event times of back-to-back
whole calls, median / min / max over the rotations; `ratio` is against `whole (1st)` of the same shape and P.V.

"""


def build(pv, B):
    pages_per = NKEYS // PAGE
    P = B * pages_per
    gen = torch.Generator(device="cuda").manual_seed(0)
    k = torch.randn(P, HK, PAGE, D, generator=gen, device="cuda", dtype=torch.float16)
    v = torch.randn(P, HK, PAGE, D, generator=gen, device="cuda", dtype=torch.float16)
    table = torch.randperm(P, generator=torch.Generator().manual_seed(1)).to(torch.int32).view(B, pages_per).cuda()
    lens = torch.full((B,), NKEYS, dtype=torch.int32, device="cuda")
    return sa.SagePagedKVCache.prepare(k, v, table, lens, pv=pv), table, lens


def restricted(table, Ts, window):
    """the table rows shifted to each sequence's first page inside the window, and the lengths from there"""
    keep = [min(NKEYS, -(-(window + t - 1) // PAGE) * PAGE) for t in Ts]
    width = max(keep) // PAGE
    rows = [torch.nn.functional.pad(table[b, (NKEYS - n) // PAGE:], (0, width - n // PAGE)) for b, n in enumerate(keep)]
    return torch.stack(rows).contiguous(), torch.tensor(keep, dtype=torch.int32, device="cuda")


def measure(pv, shape, rotations):
    Ts = [1] * 8 if shape == "decode" else [CHUNK] + [1] * 63
    B, total = len(Ts), sum(Ts)
    cache, table, lens = build(pv, B)
    variants = {}
    if shape == "decode":
        q = fold(torch.randn(B, 1, HQ, D, device="cuda", dtype=torch.float16), G)
        whole = lambda: sa.sageattn_splitkv_paged(q, cache, table, lens, num_splits=S, causal=True, q_fold=G)  # noqa: E731
        for w in (1024, 4096):
            rt, rl = restricted(table, Ts, w)
            variants[f"window {w}"] = lambda w=w: sa.sageattn_splitkv_paged_window(q, cache, table, lens, w, num_splits=S, q_fold=G)
            variants[f"restricted to window {w}"] = lambda rt=rt, rl=rl: sa.sageattn_splitkv_paged(
                q, cache, rt, rl, num_splits=S, causal=True, q_fold=G)
    else:
        q = torch.randn(total, HQ, D, device="cuda", dtype=torch.float16)
        cu = torch.tensor([0] + torch.tensor(Ts).cumsum(0).tolist(), dtype=torch.int32, device="cuda")
        plan = sa.ragged_q_plan(cu, total, G)
        whole = lambda: sa.sageattn_splitkv_paged_ragged(q, cache, table, lens, cu, plan=plan, num_splits=S, q_fold=G)  # noqa: E731
        for w in (1024, 4096):
            rt, rl = restricted(table, Ts, w)
            variants[f"window {w}"] = lambda w=w: sa.sageattn_splitkv_paged_ragged_window(
                q, cache, table, lens, cu, w, plan=plan, num_splits=S, q_fold=G)
            variants[f"restricted to window {w}"] = lambda rt=rt, rl=rl: sa.sageattn_splitkv_paged_ragged(
                q, cache, rt, rl, cu, plan=plan, num_splits=S, q_fold=G)
    variants = {"whole (1st)": whole, **variants, "whole (2nd)": whole}
    times = {name: [] for name in variants}
    for _ in range(rotations):
        for name, fn in variants.items():
            times[name].append(timed(fn, 20))
    return {name: (statistics.median(ts), min(ts), max(ts)) for name, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window.md"))
    ap.add_argument("--rotations", type=int, default=5)
    a = ap.parse_args()
    lines = ["| shape | P.V | variant | median us | min | max | ratio |", "|---|---|---|---|---|---|---|"]
    for shape in ("decode", "mixed"):
        for pv in ("fp16", "fp8"):
            rows = measure(pv, shape, a.rotations)
            for name, (med, lo, hi) in rows.items():
                lines.append(f"| {shape} | {pv} | {name} | {med:.1f} | {lo:.1f} | {hi:.1f} | {med / rows['whole (1st)'][0]:.3f} |")
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(HEAD + text)


if __name__ == "__main__":
    main()
