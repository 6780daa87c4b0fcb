#!/usr/bin/env python3
r"""Compare the gfx950 device code of two builds function by function: do the kernels a change was not meant to touch keep
their instruction streams?

    python tools/cmp_kernel_disasm.py OLD NEW [--filter REGEX] [--rename REGEX=REPL ...]

OLD and NEW are object files (sage_attn.o ...) or directories of them (csrc/ of two builds; objects are matched by name).
Every device function is disassembled (llvm-objdump -d, no raw bytes), addresses and branch-target labels are dropped, and the
remaining text -- mnemonics, registers, immediates, in order; not the padding behind a function's end -- is compared.  Prints one line per object with the number of
identical functions and names every function that differs or exists on one side only; exit status 1 if there is any such.

Functions are matched by mangled name.  Where a change renames kernels, --rename REGEX=REPL (repeatable, applied in order with
re.sub to OLD's names before matching) maps the old names to the new ones.  The predictor kernels of sage_sparge.hip lost their
_kvlen twins to a trailing template flag KVLEN; to compare against a build from before that:

    --rename '(block_(?:pool_sim|select)_kernelI.*)EEvNS_(\d+(?:Pool|Select)ParamsE)$=\1Lb0EEEvNS_\2'
    --rename '27block_pool_sim_kvlen_kernel(I.*)EEvNS_13PoolLenParamsE$=21block_pool_sim_kernel\1Lb1EEEvNS_10PoolParamsE'
    --rename '25block_select_kvlen_kernel(I.*)EEvNS_15SelectLenParamsE$=19block_select_kernel\1Lb1EEEvNS_12SelectParamsE'

(the first gives block_*_kernel<...> the flag false; the twins take one substitution each, because a mangled name spells out
the lengths of the kernel's and the parameter struct's names).  The calibration kernels of sage_calib.hip gained the same flag;
against a build from before that:

    --rename '(16tile_mass_kernelILi\d+ELb[01]E)EEvNS_10MassParamsE$=\1Lb0EEEvNS_10MassParamsE'
    --rename '18plan_recall_kernelENS_12RecallParamsE$=18plan_recall_kernelILb0EEEvNS_12RecallParamsE'

The split-KV merge kernels were folded the same way (splitkv_causal_merge_kernel<BF16, MAXC> became
splitkv_merge_kernel<BF16, MAXC, true>, the other one <BF16, MAXC, false>); against a build from before that:

    --rename '(20splitkv_merge_kernelILb[01]ELi\d+E)EEvNS_10AttnParamsEi$=\1Lb0EEEvNS_10AttnParamsEi'
    --rename '27splitkv_causal_merge_kernel(ILb[01]ELi\d+E)EEvNS_10AttnParamsEi$=20splitkv_merge_kernel\1Lb1EEEvNS_10AttnParamsEi'

The causal instantiations moved from sage_attn_splitkv_causal.o to sage_attn_splitkv.o with that.  Between two directories a
function that one object lost and another gained is compared across the two and reported as "moved".

The five K and K/V pre-pass kernels of sage_quant.hip (k_mean_partial, kv_partial, k_quant_stream, kv_quant, kv_quant_stream)
lost their _kvlen twins to a trailing template flag KVLEN and a trailing argument KvLens<KVLEN>; against a build from before
that:

    --rename '((?:21k_mean_partial|17kv_partial)_kernelI.*E)EEv(.*)$=\1Lb0EEEv\2NS_6KvLensIXT1_EEE'
    --rename '((?:21k_quant_stream|15kv_quant|22kv_quant_stream)_kernelI.*E)EEv(.*)$=\1Lb0EEEv\2NS_6KvLensIXT2_EEE'
    --rename '27k_mean_partial_kvlen_kernel(I.*E)EEv(.*)PKi$=21k_mean_partial_kernel\1Lb1EEEv\2NS_6KvLensIXT1_EEE'
    --rename '23kv_partial_kvlen_kernel(I.*E)EEv(.*)PKi$=17kv_partial_kernel\1Lb1EEEv\2NS_6KvLensIXT1_EEE'
    --rename '27k_quant_stream_kvlen_kernel(I.*E)EEv(.*)PKi$=21k_quant_stream_kernel\1Lb1EEEv\2NS_6KvLensIXT2_EEE'
    --rename '21kv_quant_kvlen_kernel(I.*E)EEv(.*)PKi$=15kv_quant_kernel\1Lb1EEEv\2NS_6KvLensIXT2_EEE'
    --rename '28kv_quant_stream_kvlen_kernel(I.*E)EEv(.*)PKi$=22kv_quant_stream_kernel\1Lb1EEEv\2NS_6KvLensIXT2_EEE'

(the first two give the kernels without lengths the flag false and the argument, the others rename the twins, whose last
argument was the pointer, PKi.  A mangled name spells the argument's type as "KvLens of the kernel's template parameter n":
XT1_ is the third parameter of the two partial kernels, XT2_ the fourth of the three quantizers)."""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sageattention_amd import _build  # noqa: E402

OBJDUMP = os.path.join(os.path.dirname(os.path.dirname(_build.HIPCC)), "lib", "llvm", "bin", "llvm-objdump")


def functions(obj):
    """{mangled name: [normalised instruction text]} of the gfx950 code object inside ``obj``"""
    tmp = tempfile.mkdtemp(prefix="sage_dis_")
    try:
        local = os.path.join(tmp, "o.o")
        shutil.copy(obj, local)
        subprocess.run([OBJDUMP, "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
        dev = glob.glob(local + ".*" + _build.ARCH)
        if not dev:  # host code only (sage_op.o)
            return {}
        text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", dev[0]], stdout=subprocess.PIPE, text=True, check=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:$", line)
        if m:
            name = m.group(1)
            if not name.startswith("L"):  # a function, not a local label
                out[name] = []
                cur = out[name]
            continue
        if name is None or not line.strip():
            continue
        ins = re.sub(r"^\s*[0-9a-f]+:\s*", "", line)      # address column
        ins = re.sub(r"//.*$", "", ins).strip()            # objdump's comment (address, encoding)
        ins = re.sub(r"<[^>]+>", "<label>", ins)           # branch targets by name
        if ins:
            cur.append(ins)
    # what follows a function's last instruction up to the next symbol: alignment, objdump's "...", and zero dwords, which
    # decode as this v_cndmask (no function ends with one: its last instruction is s_endpgm or a branch)
    for ins in out.values():
        while ins and ins[-1] in ("s_nop 0", "s_code_end", "...", "v_cndmask_b32_e32 v0, s0, v0, vcc"):
            ins.pop()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--filter", default="", help="only functions whose mangled name matches this regex")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL",
                    help="re.sub applied to OLD's mangled names before matching (repeatable, in order)")
    a = ap.parse_args()
    if os.path.isdir(a.old):
        names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(a.old, "*.o")))
        pairs = [(os.path.join(a.old, n), os.path.join(a.new, n)) for n in names if os.path.exists(os.path.join(a.new, n))]
    else:
        pairs = [(a.old, a.new)]
    bad = 0
    both = []
    for old, new in pairs:
        fo, fn = functions(old), functions(new)
        for r in a.rename:
            rx, repl = r.split("=", 1)
            fo = {re.sub(rx, repl, n): ins for n, ins in fo.items()}
        both.append((os.path.basename(old), fo, fn))
    # a function that one object lost and another gained: {name: (object, instructions)} on either side
    lost = {n: (obj, fo[n]) for obj, fo, fn in both for n in fo if n not in fn}
    gained = {n: (obj, fn[n]) for obj, fo, fn in both for n in fn if n not in fo}
    moved = sorted(n for n in set(lost) & set(gained) if re.search(a.filter, n))
    for obj, fo, fn in both:
        keep = [n for n in sorted(set(fo) | set(fn)) if re.search(a.filter, n) and n not in moved]
        same = [n for n in keep if n in fo and n in fn and fo[n] == fn[n]]
        print(f"{obj}: {len(same)} of {len(keep)} functions identical ({sum(len(fo[n]) for n in same)} instructions)")
        for n in keep:
            if n in same:
                continue
            bad += 1
            what = "only in OLD" if n not in fn else "only in NEW" if n not in fo else \
                f"DIFFERS ({len(fo[n])} -> {len(fn[n])} instructions)"
            print(f"  {n}: {what}")
    for n in moved:
        (src, io), (dst, ino) = lost[n], gained[n]
        bad += io != ino
        print(f"moved {src} -> {dst}: {n}: " +
              (f"identical ({len(io)} instructions)" if io == ino else f"DIFFERS ({len(io)} -> {len(ino)} instructions)"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
