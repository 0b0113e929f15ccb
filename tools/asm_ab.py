"""Per-kernel comparison of two trees' gfx950 instruction streams (the no-GPU half of an A/B: an identical stream needs no timing).

    hipcc <build.py FLAGS> --cuda-device-only -S csrc/<file>.hip -o <dir>/<file>.s      for both trees, then
    python tools/asm_ab.py <parent dir> <new dir> [file ...]

Per kernel symbol: IDENTICAL / DIFFERS after stripping labels, directives and comments, instruction counts, registers, LDS, scratch
and the instruction classes that decide a conv kernel's speed."""
import os
import re
import subprocess
import sys


def kernels(path):
    """{demangled kernel name: (instructions, {metadata})} of one .s file"""
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\s*s_endpgm\b(.*?)^\s*\.end_amdhsa_kernel", txt, re.S | re.M):
        sym, body, tail = m.groups()
        ins = []
        for line in body.split("\n"):
            line = line.split(";")[0].strip()
            if not line or line.endswith(":") or line.startswith("."):
                continue
            ins.append(re.sub(r"\s+", " ", line))
        meta = {k: int(v) for k, v in re.findall(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|group_segment_fixed_size|private_segment_fixed_size|accum_offset) (\d+)", tail)}
        out[sym] = (ins, meta)
    if not out:
        return out
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True).stdout.split("\n")
    return {re.sub(r"^void |\(ffp::ConvArgs\)$|ffp::|\(anonymous namespace\)::", "", n): v for n, v in zip(names, out.values())}


def count(ins, pat):
    return sum(1 for i in ins if re.match(pat, i))


CLASSES = [("mfma", r"v_mfma"), ("ds_read", r"ds_read"), ("ds_write", r"ds_write"), ("buffer_load", r"buffer_load"), ("global_load", r"global_load"),
           ("store", r"(buffer|global)_store"), ("s_barrier", r"s_barrier"), ("v_exp", r"v_exp"), ("v_max", r"v_max")]


def main():
    pa, pb = sys.argv[1], sys.argv[2]
    files = sys.argv[3:] or sorted(f[:-2] for f in os.listdir(pb) if f.endswith(".s"))
    same = differ = 0
    for f in files:
        ka, kb = kernels(os.path.join(pa, f + ".s")), kernels(os.path.join(pb, f + ".s"))
        for name in sorted(set(ka) | set(kb)):
            if name not in ka or name not in kb:
                print(f"{f}: {name}: only in the {'new' if name in kb else 'parent'} tree")
                continue
            (ia, ma), (ib, mb) = ka[name], kb[name]
            ident = ia == ib
            same += ident
            differ += not ident
            print(f"{f}: {name}: {'IDENTICAL' if ident else 'DIFFERS'}  instructions {len(ia)} -> {len(ib)}")
            print("    " + "  ".join(f"{k.replace('next_free_', '').replace('_segment_fixed_size', '')} {ma.get(k, 0)} -> {mb.get(k, 0)}"
                                     for k in ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")))
            if not ident:
                print("    " + "  ".join(f"{c} {count(ia, p)} -> {count(ib, p)}" for c, p in CLASSES))
    print(f"# {same} identical, {differ} differ")


if __name__ == "__main__":
    main()
