"""Dev tool: per-stage census of register-file shuffling in one kernel's ISA (sibling of tools/static_profile.py).

usage: python tools/regfile_census.py [kernel-substring] [--stamps] [--asm FILE] [--segments] [extra hipcc flags]

Compiles csrc/meshenv_hip.hip with the shipped flags to gfx950 assembly (device code only; --asm FILE reads a listing made
earlier instead) and counts, for the named kernel, static instructions by the classes DESIGN.md section 5 tabulates:

  fp64     v_*_f64 arithmetic (add / mul / fma / div_* / rcp / rsq / min / max / cmp / cvt ...)
  v_mov    v_mov_b32 / v_mov_b64 / v_accvgpr_*      (VGPR <- VGPR / SGPR / literal)
  s_mov    s_mov_b32 / s_mov_b64 / s_movk_i32       (SGPR <- SGPR / literal, exec copies included)
  lane     v_readlane / v_readfirstlane / v_writelane   (moves between the two register files, SGPR spills included)
  s_nop    s_nop
  other    everything else

A stage ends at the workgroup barrier (s_barrier: phase 1 | phase 2 in the CU-group kernels), at a `; wave barrier` marker
(wave_sync() of csrc/meshenv_kernels.h) and, with --stamps (-DMESHENV_STAMPS), at an s_memrealtime of a MESHENV_STAMP site.
Stages are numbered in the order of the listing, which is the compiler's block layout, not the order of execution; the
table groups them into "in front of the barrier" and "behind the barrier" and prints the single segments with --segments.
Classes only: nothing here looks for a particular instruction beyond the prefixes above."""
import collections, os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["fp64", "v_mov", "s_mov", "lane", "s_nop", "other"]
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math",
         "--offload-arch=gfx950", "-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None",
         "-mllvm", "-amdgpu-kernarg-preload-count=16", "--cuda-device-only", "-S"]


def klass(op):
    if op.startswith(("v_readlane", "v_readfirstlane", "v_writelane")): return "lane"
    if op.startswith(("v_mov_", "v_accvgpr_")): return "v_mov"
    if op.startswith(("s_mov_b", "s_movk_")): return "s_mov"
    if op == "s_nop": return "s_nop"
    if op.startswith("v_") and (op.endswith("_f64") or "_f64_" in op): return "fp64"
    return "other"


def listing(argv):
    if "--asm" in argv:
        return open(argv[argv.index("--asm") + 1]).read().splitlines()
    tmp = "/tmp/meshenv_static"; os.makedirs(tmp, exist_ok=True)
    extra = [a for a in argv if a.startswith("-") and a not in ("--stamps", "--segments")]
    if "--stamps" in argv: extra.append("-DMESHENV_STAMPS")
    out = os.path.join(tmp, "census.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", *FLAGS, *extra, "-o", out,
                           os.path.join(ROOT, "reinforcementlearning4meshgeneration_amd", "csrc", "meshenv_hip.hip")], stderr=subprocess.DEVNULL)
    return open(out).read().splitlines()


def census(lines, kern):
    """[(what ended the segment, Counter by class)] of the kernel whose mangled name contains kern"""
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(kern) + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    segs, cur = [], collections.Counter()
    for l in lines[start + 1:end]:
        s = l.strip()
        if s.startswith("; wave barrier"):
            segs.append(("wave barrier", cur)); cur = collections.Counter(); continue
        m = re.match(r"^([a-z][a-z_0-9]*)\b", s)
        if not m or s.endswith(":") or s.startswith((".", ";")): continue
        op = m.group(1)
        cur[klass(op)] += 1
        if op == "s_barrier":
            segs.append(("s_barrier", cur)); cur = collections.Counter()
        elif op.startswith("s_memrealtime"):
            segs.append(("stamp", cur)); cur = collections.Counter()
    segs.append(("end", cur))
    return lines[start].rstrip(":"), segs


def row(name, c):
    tot = sum(c.values())
    shuffle = c["v_mov"] + c["s_mov"] + c["lane"]
    return (f"{name:28s} {tot:6d} " + " ".join(f"{c[k]:6d}" for k in CLASSES) + f" {shuffle:8d}"
            + "   " + " ".join(f"{100 * c[k] / max(tot, 1):5.1f}%" for k in CLASSES[:5]))


def main(argv):
    names = [a for i, a in enumerate(argv) if not a.startswith("-") and (i == 0 or argv[i - 1] != "--asm")]
    kern = names[0] if names else "k_step_groupILi16ELb1ELb0ELb1E"   # the headline kernel: k_step_group<16, true, false, true>
    name, segs = census(listing(argv), kern)
    print(name)
    print(f"{'stage':28s} {'all':>6s} " + " ".join(f"{k:>6s}" for k in CLASSES) + " mov+lane   share of the stage: " + " ".join(CLASSES[:5]))
    nb = next((i for i, (w, _) in enumerate(segs) if w == "s_barrier"), None)
    if "--segments" in argv or nb is None:
        for i, (w, c) in enumerate(segs):
            print(row(f"{i:3d} (ends at {w})", c))
    if nb is not None:
        front, behind = collections.Counter(), collections.Counter()
        for w, c in segs[:nb + 1]: front.update(c)
        for w, c in segs[nb + 1:]: behind.update(c)
        print(row("in front of the barrier", front))
        print(row("behind the barrier", behind))
    whole = collections.Counter()
    for w, c in segs: whole.update(c)
    print(row("kernel", whole))


if __name__ == "__main__":
    main(sys.argv[1:])
