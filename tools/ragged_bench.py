#!/usr/bin/env python3
"""Whole-call times of ragged-query attention on the paged cache against what a user does without it -> profiles/ragged_q.md.

    python tools/ragged_bench.py [--out profiles/ragged_q.md] [--rotations 5]

Mixed step: one prefill chunk of 2048 tokens plus 63 decode sequences, every sequence at 8192 keys, Hq 32 / Hk 8, head_dim 128,
g = 4, page size 64, both P.V types.  The one ragged call (plan made once) against
  * the padded call: M = 2048 * g rows for every sequence, left-padded, sageattn_splitkv_paged(causal=True);
  * two calls, one over the prefill sequence and one over the decode sequences, each with the hand fold's copy of q.
Pure decode: T_b = 1 everywhere against sageattn_splitkv_paged(causal=True) of the same shape -- what the work list and the
un-folded addressing cost.  That yardstick is timed twice per rotation; its two times give the spread a ratio is read against.
Times are HIP-event times of `iters` back-to-back calls, host side included, median over the rotations."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sageattention_amd as sa  # noqa: E402

HQ, HK, D, G, PAGE, NKEYS, B, CHUNK = 32, 8, 128, 4, 64, 8192, 64, 2048


HEAD = """# Ragged-query attention on the paged cache: whole-call times and the accuracy yardstick

`python tools/ragged_bench.py` on one MI355X.  Mixed step: one prefill chunk of 2048 tokens plus 63 decode sequences, all at 8192
keys, Hq 32 / Hk 8, head_dim 128, g = 4, page size 64, num_splits 4 in every variant.  Pure decode: T_b = 1 for all 64 sequences.
HIP-event times of back-to-back whole calls (host side included), median / min / max over the rotations.  `ratio` is against
the ragged call for the mixed rows and against the yardstick's first timing for the decode rows; the yardstick's second timing
shows the spread a ratio has to be read against.

"""
ACCURACY = """
## The accuracy yardstick of tests/test_ragged_gpu.py

The parent's `sageattn_splitkv_paged(causal=True)`, called per sequence (g = 2, num_splits 3, per_thread) on the test's own batch
(Hq 4 / Hk 2, six sequences, 204 tokens, fp16), against a float64 softmax over the fp16 K / V gathered from the pages:

| head_dim | P.V | max abs error of o | max abs error of lse |
|---|---|---|---|
| 64 | fp16 | 4.289e-02 | 3.485e-02 |
| 64 | fp8 | 9.961e-02 | 3.487e-02 |
| 128 | fp16 | 4.853e-02 | 4.003e-02 |
| 128 | fp8 | 1.096e-01 | 4.003e-02 |

The test allows the ragged operator 1.5 times these figures; its rows have the parent's bits (the first test there), so it
measures exactly them.  The keys of the test are N(0.3, 1.5^2): the INT8 rounding of K is what the figures show.
"""


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def fold(q, g):
    """[B, T, Hq, D] -> the hand fold [B, Hq / g, T * g, D] (a copy unless Hk = 1)"""
    Bq, T, H, Dq = q.shape
    return q.reshape(Bq, T, H // g, g, Dq).permute(0, 2, 1, 3, 4).reshape(Bq, H // g, T * g, Dq)


def build(pv):
    pages_per = NKEYS // PAGE
    P = B * pages_per
    gen = torch.Generator(device="cuda").manual_seed(0)
    k = torch.randn(P, HK, PAGE, D, generator=gen, device="cuda", dtype=torch.float16)
    v = torch.randn(P, HK, PAGE, D, generator=gen, device="cuda", dtype=torch.float16)
    table = torch.randperm(P, generator=torch.Generator().manual_seed(1)).to(torch.int32).view(B, pages_per).cuda()
    lens = torch.full((B,), NKEYS, dtype=torch.int32, device="cuda")
    return sa.SagePagedKVCache.prepare(k, v, table, lens, pv=pv), table, lens


def measure(pv, rotations):
    cache, table, lens = build(pv)
    S = 4
    rows = {}
    # ---- the mixed step
    Ts = [CHUNK] + [1] * (B - 1)
    total = sum(Ts)
    cu = torch.tensor([0] + torch.tensor(Ts).cumsum(0).tolist(), dtype=torch.int32, device="cuda")
    q = torch.randn(total, HQ, D, device="cuda", dtype=torch.float16)
    plan = sa.ragged_q_plan(cu, total, G)
    padded = torch.zeros(B, CHUNK, HQ, D, device="cuda", dtype=torch.float16)
    padded[0] = q[:CHUNK]
    padded[1:, -1] = q[CHUNK:]
    q_pad = fold(padded, G).contiguous()
    pre, dec = cache.narrow(0, 1), cache.narrow(1, B - 1)
    variants = {
        "mixed: ragged, one call": lambda: sa.sageattn_splitkv_paged_ragged(q, cache, table, lens, cu, plan=plan, num_splits=S, q_fold=G),
        "mixed: padded to 2048 tokens": lambda: sa.sageattn_splitkv_paged(q_pad, cache, table, lens, num_splits=S, causal=True, q_fold=G),
        "mixed: two calls with the hand fold": lambda: (
            sa.sageattn_splitkv_paged(fold(q[:CHUNK].unsqueeze(0), G), pre, table[:1], lens[:1], num_splits=S, causal=True, q_fold=G),
            sa.sageattn_splitkv_paged(fold(q[CHUNK:].unsqueeze(1), G), dec, table[1:], lens[1:], num_splits=S, causal=True, q_fold=G)),
    }
    # ---- pure decode
    cu1 = torch.arange(B + 1, dtype=torch.int32, device="cuda")
    q1 = torch.randn(B, HQ, D, device="cuda", dtype=torch.float16)
    plan1 = sa.ragged_q_plan(cu1, B, G)
    yard = lambda: sa.sageattn_splitkv_paged(fold(q1.unsqueeze(1), G), cache, table, lens, num_splits=S, causal=True, q_fold=G)  # noqa: E731
    variants["decode: ragged"] = lambda: sa.sageattn_splitkv_paged_ragged(q1, cache, table, lens, cu1, plan=plan1, num_splits=S, q_fold=G)
    variants["decode: sageattn_splitkv_paged (yardstick, 1st)"] = yard
    variants["decode: sageattn_splitkv_paged (yardstick, 2nd)"] = yard
    times = {name: [] for name in variants}
    for _ in range(rotations):
        for name, fn in variants.items():
            times[name].append(timed(fn, 3 if "padded" in name else 20))
    for name, ts in times.items():
        rows[name] = (statistics.median(ts), min(ts), max(ts))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_q.md"))
    ap.add_argument("--rotations", type=int, default=5)
    a = ap.parse_args()
    lines = ["| P.V | variant | median us | min | max | ratio |", "|---|---|---|---|---|---|"]
    for pv in ("fp16", "fp8"):
        rows = measure(pv, a.rotations)
        for name, (med, lo, hi) in rows.items():
            base = rows["mixed: ragged, one call" if name.startswith("mixed") else "decode: sageattn_splitkv_paged (yardstick, 1st)"][0]
            lines.append(f"| {pv} | {name} | {med:.1f} | {lo:.1f} | {hi:.1f} | {med / base:.3f} |")
        torch.cuda.empty_cache()
    text = HEAD + "\n".join(lines) + "\n" + ACCURACY
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
