#!/usr/bin/env python3
"""Per-batch key lengths on the block-sparse and Sparge paths, whole calls timed in ONE process with alternating windows:
every variant of a comparison is timed in turn, `--repeats` times round robin, each window a warm-up and then HIP events
around enough calls to last about `--window-ms`.  A time is the median over the windows; a ratio is the median of the
per-round ratios with their least and greatest value beside it.

The yardstick is the same operator WITHOUT kv_lens running on a library built from the parent commit (--parent-lib: its
libsageattn_hip.so; the Python layer is this commit's, which calls the ops and entry points it called before).  It is timed
twice in every rotation ("parent again"), so that its own spread is on the page.  Without --parent-lib the yardstick is this
commit's library, and the page says so.

  (a) full lengths, kv_lens = N everywhere: (4,32,8192,128) and (4,32,2048,64), map density 1 and 1/4, FP16 and FP8 PV
  (b) a guidance-style batch (2,40,N,128), the second batch a few hundred keys shorter: sageattn_sparge, topk=0.25, keep_last=4
  (c) lengths [8192,6144,4096,2048] at (4,32,8192,128) under an all-ones map, beside the dense sageattn_kvlen on the same lengths
  (d) `python bench.py` figures of the parent commit and of this one, taken alternately on one machine by the caller and
      handed in as files of JSON lines (--bench-parent, --bench-branch); absent, the section says "not measured"
Random inputs; rows >= len_b of K and V hold NaN where lengths are ragged, as a padded batch may.

usage: sparse_kvlen_bench.py [--parent-lib PATH] [--repeats 5] [--window-ms 200] [--sections a,b,c]
                             [--bench-parent p.jsonl --bench-branch b.jsonl] [--commit HASH] [--out profiles/sparse_kvlen.md]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import sageattention_amd as sa  # noqa: E402
from sageattention_amd import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default="")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window-ms", type=float, default=200.0)
ap.add_argument("--sections", default="a,b,c")
ap.add_argument("--guidance-n", type=int, default=8192 + 512)
ap.add_argument("--bench-parent", default="")
ap.add_argument("--bench-branch", default="")
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()
lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


if not torch.cuda.is_available():
    sys.exit("sparse_kvlen_bench.py measures on the GPU: none is visible")

THIS = L.lib()
PARENT = THIS
if a.parent_lib:
    PARENT = L.bind(ctypes.CDLL(os.path.abspath(a.parent_lib)))


def on_parent(fn):
    """fn, with the package bound to the parent's library for the duration of the call"""
    def run():
        L._lib = PARENT
        try:
            return fn()
        finally:
            L._lib = THIS
    return run


def events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n  # ms per call


def rounds(variants):
    """variants: name -> callable.  Round robin, a.repeats rounds -> name -> [ms per call of every round]"""
    calls = {}
    for name, fn in variants.items():  # first launches load code objects; then size the window of this variant
        for _ in range(3):
            fn()
        calls[name] = max(10, int(a.window_ms / max(events(fn, 5), 1e-3)))
    out = {name: [] for name in variants}
    for _ in range(a.repeats):
        for name, fn in variants.items():
            for _ in range(3):
                fn()
            out[name].append(events(fn, calls[name]))
    return out


def med(ts):
    return statistics.median(ts)


def ratio(ts, base):
    r = [x / y for x, y in zip(ts, base)]
    return f"{med(r):.3f} ({min(r):.3f} .. {max(r):.3f})"


def make(B, H, M, N, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, H, M, D, generator=g, device="cuda").half()
    k = torch.randn(B, H, N, D, generator=g, device="cuda").half()
    v = torch.randn(B, H, N, D, generator=g, device="cuda").half()
    return q, k, v


def poison(k, v, lens):
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
        v[b, :, n:] = float("nan")


def random_map(B, H, M, N, density, seed):
    nqb, ntk = (M + 127) // 128, (N + 63) // 64
    if density >= 1:
        return torch.ones(B, H, nqb, ntk, dtype=torch.bool, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    bm = torch.rand(B, H, nqb, ntk, generator=g, device="cuda") < density
    bm[..., 0] = True  # no empty q-block
    return bm


def bench_lines(path):
    return [json.loads(ln) for ln in (x.strip() for x in open(path)) if ln.startswith("{")]


sections = a.sections.split(",")
emit("# kv_lens on the block-sparse and Sparge paths: times on MI355X")
emit()
emit(f"commit {a.commit or 'unknown'}; tools/sparse_kvlen_bench.py, one process, the variants of a comparison timed round robin in")
emit(f"{a.repeats} rounds, a window = 3 warm-up calls and HIP events around about {a.window_ms:.0f} ms of calls.  fp16 inputs, per-thread")
emit("scales, whole calls (pre-pass + attention, for Sparge also the predictor).  Times: median over the rounds.  Ratios: median")
emit("of the per-round ratios (least .. greatest).")
emit("\"parent\" is the same operator without kv_lens on " + ("a library built from the parent commit" if a.parent_lib else
     "THIS commit's library (no --parent-lib was given)") + "; \"parent again\" is that")
emit("call timed a second time in the same rotation: its ratio to \"parent\" is the spread a ratio has to leave before it says anything.")

if "a" in sections:
    emit()
    emit("## (a) full lengths: the cost of the keyword")
    emit()
    emit("kv_lens = N for every batch, a plan compacted once; o and lse of the two calls are compared bit for bit first.  What the")
    emit("keyword adds to a call: the length-aware pre-pass twin, one scalar load of the length per workgroup (a batch of full length")
    emit("does not walk its list), and the empty-rows launch of the kvlen form in the place of the other one.")
    emit()
    emit("| shape (B,H,N,D) | density | PV | parent ms | kv_lens ms | kv_lens / parent | parent again / parent | bits |")
    emit("|---|---|---|---|---|---|---|---|")
    for (B, H, N, D) in ((4, 32, 8192, 128), (4, 32, 2048, 64)):
        q, k, v = make(B, H, N, N, D, N + D)
        full = torch.full((B,), N, dtype=torch.int32, device="cuda")
        for density in (1.0, 0.25):
            plan = sa.block_sparse_plan(random_map(B, H, N, N, density, 3), N, N)
            for pv in ("fp16", "fp8"):
                o0, l0 = on_parent(lambda: sa.sageattn_block_sparse(q, k, v, plan, pv=pv, return_lse=True))()
                o1, l1 = sa.sageattn_block_sparse(q, k, v, plan, pv=pv, return_lse=True, kv_lens=full)
                same = "equal" if torch.equal(o0, o1) and torch.equal(l0, l1) else "DIFFERENT"
                del o0, l0, o1, l1
                par = on_parent(lambda: sa.sageattn_block_sparse(q, k, v, plan, pv=pv))
                t = rounds({"parent": par, "kvlen": lambda: sa.sageattn_block_sparse(q, k, v, plan, pv=pv, kv_lens=full),
                            "again": par})
                emit(f"| ({B},{H},{N},{D}) | {density:g} | {pv} | {med(t['parent']):.4f} | {med(t['kvlen']):.4f} | "
                     f"{ratio(t['kvlen'], t['parent'])} | {ratio(t['again'], t['parent'])} | {same} |")
        del q, k, v

if "b" in sections:
    emit()
    emit("## (b) a guidance-style batch through sageattn_sparge")
    emit()
    B, H, N, D = 2, 40, a.guidance_n, 128
    lens = [N, N - 300]
    emit(f"({B},{H},{N},{D}), kv_lens = {lens} (the second prompt 300 tokens shorter), topk=0.25, keep_last=4.  \"parent\" runs the")
    emit("same call without kv_lens on finite K and V: it pools, selects and attends the padding, and its keep_last pins padding blocks.")
    emit()
    emit("| PV | parent ms | kv_lens ms | kv_lens / parent | parent again / parent |")
    emit("|---|---|---|---|---|")
    q, k, v = make(B, H, N, N, D, 5)
    kp, vp = k.clone(), v.clone()
    poison(kp, vp, lens)
    kv_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    kw = dict(topk=0.25, keep_last=4)
    for pv in ("fp16", "fp8"):
        par = on_parent(lambda: sa.sageattn_sparge(q, k, v, pv=pv, **kw))
        t = rounds({"parent": par, "kvlen": lambda: sa.sageattn_sparge(q, kp, vp, pv=pv, kv_lens=kv_lens, **kw), "again": par})
        emit(f"| {pv} | {med(t['parent']):.4f} | {med(t['kvlen']):.4f} | {ratio(t['kvlen'], t['parent'])} | {ratio(t['again'], t['parent'])} |")
    del q, k, v, kp, vp

if "c" in sections:
    emit()
    emit("## (c) ragged lengths under an all-ones map, beside the dense sageattn_kvlen")
    emit()
    B, H, N, D = 4, 32, 8192, 128
    lens = [8192, 6144, 4096, 2048]
    emit(f"({B},{H},{N},{D}), kv_lens = {lens}: sum(len) / (B N) = {sum(lens) / (B * N):.3f} of the tiles.  Every list of a shortened batch is")
    emit("walked by the clip (128 entries: one chunk).  \"parent\" = the block-sparse call without kv_lens on finite K and V, all tiles.")
    emit()
    emit("| PV | parent ms | sparse kv_lens ms | dense sageattn_kvlen ms | sparse kv_lens / parent | sparse kv_lens / dense kvlen | parent again / parent |")
    emit("|---|---|---|---|---|---|---|")
    q, k, v = make(B, H, N, N, D, 7)
    kp, vp = k.clone(), v.clone()
    poison(kp, vp, lens)
    kv_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    plan = sa.block_sparse_plan(random_map(B, H, N, N, 1.0, 0), N, N)
    for pv in ("fp16", "fp8"):
        par = on_parent(lambda: sa.sageattn_block_sparse(q, k, v, plan, pv=pv))
        t = rounds({"parent": par, "kvlen": lambda: sa.sageattn_block_sparse(q, kp, vp, plan, pv=pv, kv_lens=kv_lens),
                    "dense": lambda: sa.sageattn_kvlen(q, kp, vp, kv_lens, pv=pv), "again": par})
        emit(f"| {pv} | {med(t['parent']):.4f} | {med(t['kvlen']):.4f} | {med(t['dense']):.4f} | {ratio(t['kvlen'], t['parent'])} | "
             f"{ratio(t['kvlen'], t['dense'])} | {ratio(t['again'], t['parent'])} |")
    del q, k, v, kp, vp

emit()
emit("## (d) calls without kv_lens: bench.py on the parent commit and on this one")
emit()
if a.bench_parent and a.bench_branch:
    par, br = bench_lines(a.bench_parent), bench_lines(a.bench_branch)
    key = "value"
    emit(f"`python bench.py --gpus 1` run alternately (parent, branch, parent, ...) on one machine, {len(par)} runs each; the JSON")
    emit(f"line's `{key}` ({par[0].get('unit', '')}, {par[0].get('metric', par[0].get('name', 'headline'))}):")
    emit()
    emit("| run | parent | branch |")
    emit("|---|---|---|")
    for i, (x, y) in enumerate(zip(par, br)):
        emit(f"| {i + 1} | {x[key]} | {y[key]} |")
    pv_, bv_ = [x[key] for x in par], [y[key] for y in br]
    emit(f"| median | {med(pv_):.2f} | {med(bv_):.2f} |")
    emit()
    emit(f"parent's own spread: {min(pv_)} .. {max(pv_)} ({(max(pv_) - min(pv_)) / med(pv_) * 100:.2f} % of its median); branch median / parent")
    emit(f"median = {med(bv_) / med(pv_):.4f}.")
else:
    emit("not measured in this run (no --bench-parent / --bench-branch files).")

if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
