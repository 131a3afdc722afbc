#!/usr/bin/env python3
"""The shape of the decode GEMV loops in the ISA, read without a GPU.

    python tools/gemv_isa.py -k 'gemv_qkv_rope_kernel<unsigned short, teo::p13_t, true, true, 4, 2>'     # compile, then report
    python tools/gemv_isa.py --asm gemv.s -k p13_t                                                       # report from a kept .s
    python tools/gemv_isa.py --asm new.s --against parent.s                                              # which kernel bodies changed

Compiles teochat_amd/csrc/gemv.hip to gfx950 assembly with the Makefile's CXXFLAGS (a full compile: minutes) and, for every kernel whose
DEMANGLED name contains one of the -k substrings, prints

  * VGPRs, SGPRs, scratch bytes and the waves per SIMD the VGPRs allow (512 / VGPRs, granule 8, at most 8);
  * for every loop (a backward branch) with at least six global / buffer loads, its timeline:
        L16 / L8 / L4 / L2 / L1   a global_load_ or buffer_load_ of dwordx4 / dwordx2 / dword / ushort / ubyte
        Wn                        s_waitcnt vmcnt(n)
        vN                        N vector ALU instructions in a row (scalar, LDS and branch instructions are not shown)
    and the number of 64-bit vector address instructions in it (v_lshl_add_u64, v_mad_u64_u32 / v_mad_i64_i32, v_addc_co_u32);
  * the sha256 of the kernel's body (instructions and labels, comments and directives dropped, block labels renumbered per kernel).

--against OTHER.s compares the body digests of ALL kernels with another assembly of the same file and lists the ones that differ or exist
on one side only: the way to show that a change to the image kernels left every other instantiation as it was.

Nothing but the schedule holds the order of the loads in these loops, so this is what to run again after a compiler change.  Host only."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "teochat_amd", "csrc")

LOAD = re.compile(r"^(?:global|buffer|flat)_load_(dwordx4|dwordx3|dwordx2|dword|ushort|sshort|short_d16(?:_hi)?|ubyte|sbyte|ubyte_d16(?:_hi)?)\b")
BYTES = {"dwordx4": 16, "dwordx3": 12, "dwordx2": 8, "dword": 4, "ushort": 2, "sshort": 2, "ubyte": 1, "sbyte": 1}
ADDR64 = ("v_lshl_add_u64", "v_mad_u64_u32", "v_mad_i64_i32", "v_addc_co_u32")
BRANCH = re.compile(r"^s_c?branch\w*\s+(\.LBB\d+_\d+)")
MIN_LOADS = 6


def makefile_flags():
    """CXXFLAGS and the defaults of HIPCC / ARCH, from the Makefile that builds the library"""
    var = {}
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"^(HIPCC|ARCH|CXXFLAGS)\s*\??=\s*(.*)$", line)
        if m:
            var[m.group(1)] = m.group(2).strip()
    flags = var["CXXFLAGS"].replace("$(ARCH)", os.environ.get("ARCH", var["ARCH"]))
    return os.environ.get("HIPCC", var["HIPCC"]), flags.split()


def compile_asm(out):
    hipcc, flags = makefile_flags()
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(CSRC, "gemv.hip"), "-o", out]
    print("# " + " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)


def demangle(names):
    tool = os.path.join(os.path.dirname(os.path.realpath(makefile_flags()[0])), "..", "llvm", "bin", "llvm-cxxfilt")
    for exe in (tool, "llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([exe], input="\n".join(names), capture_output=True, text=True, check=True)
            return dict(zip(names, r.stdout.split("\n")))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def parse(path):
    """{mangled name: dict(body=[instruction and label lines], vgpr, sgpr, scratch)} for every kernel of an assembly file"""
    text = open(path).read()
    kernels, cur, name = {}, None, None
    for raw in text.split("\n"):
        line = raw.split(";", 1)[0].strip()
        m = re.match(r"^\.type\s+(\S+),@function", line)
        if m:
            name = m.group(1)
            continue
        if name and cur is None and line == name + ":":
            cur = []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                kernels[name] = dict(body=cur)
                cur, name = None, None
            elif line and (not line.startswith(".") or line.startswith(".LBB")):
                cur.append(line)
    for m in re.finditer(r"^\s+\.name:\s+(\S+)\n(.*?)(?=^\s+- \.|^\.\.\.|\Z)", text, re.S | re.M):
        k = kernels.get(m.group(1))
        if k is None:
            continue
        for key, field in (("scratch", "private_segment_fixed_size"), ("sgpr", "sgpr_count"), ("vgpr", "vgpr_count"), ("spill", "vgpr_spill_count")):
            f = re.search(r"\." + field + r":\s+(\d+)", m.group(2))
            k[key] = int(f.group(1)) if f else None
    return {n: k for n, k in kernels.items() if "vgpr" in k}


def digest(body):
    ids = {}
    def renumber(m):
        return ".L" + str(ids.setdefault(m.group(0), len(ids)))
    return hashlib.sha256("\n".join(re.sub(r"\.LBB\d+_\d+", renumber, l) for l in body).encode()).hexdigest()


def waves_per_simd(vgpr):
    return max(1, min(8, 512 // max(8, (vgpr + 7) // 8 * 8)))


def loops(body):
    """(first, last) line index of every loop: a label and the LAST backward branch to it (an outer loop, such as the walk over the row
    groups, contains its inner loops and the masked tail step behind them)"""
    at = {l[:-1]: i for i, l in enumerate(body) if l.endswith(":")}
    last = {}
    for i, l in enumerate(body):
        m = BRANCH.match(l)
        if m and at.get(m.group(1), len(body)) < i:
            last[at[m.group(1)]] = i
    return sorted(last.items())


def timeline(lines):
    toks, valu, nload, naddr = [], 0, 0, 0
    def flush():
        nonlocal valu
        if valu:
            toks.append(f"v{valu}")
            valu = 0
    for l in lines:
        op = l.split()[0] if l.split() else ""
        m = LOAD.match(l)
        if m:
            flush()
            kind = m.group(1)
            toks.append("L%d" % BYTES.get(kind, 2 if "short" in kind else 1))
            nload += 1
        elif op == "s_waitcnt":
            w = re.search(r"vmcnt\((\d+)\)", l)
            if w:
                flush()
                toks.append("W" + w.group(1))
        elif op.startswith("v_"):
            valu += 1
            naddr += op.startswith(ADDR64)
    flush()
    return toks, nload, naddr


def squeeze(toks):
    """runs of one token as `tok xN`"""
    out = []
    for t in toks:
        if out and out[-1][0] == t:
            out[-1][1] += 1
        else:
            out.append([t, 1])
    return " ".join(t if n == 1 else f"{t}x{n}" for t, n in out)


def report(name, pretty, k):
    body = k["body"]
    print(f"\n{pretty}")
    print(f"  vgpr {k['vgpr']} ({waves_per_simd(k['vgpr'])} waves/SIMD)  sgpr {k['sgpr']}  scratch {k['scratch']} B  spilled vgprs {k['spill']}  "
          f"instructions {sum(not l.endswith(':') for l in body)}")
    print(f"  sha256 {digest(body)}")
    for a, b in loops(body):
        toks, nload, naddr = timeline(body[a:b + 1])
        if nload >= MIN_LOADS:
            first_wait = next((i for i, t in enumerate(toks) if t.startswith("W")), len(toks))
            ahead = sum(t.startswith("L") for t in toks[:first_wait])
            print(f"  loop {body[a][:-1]} ({b - a} lines): {nload} loads, {ahead} ahead of the first vmcnt wait, {naddr} 64-bit vector address instructions")
            print("    " + squeeze(toks))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", help="an assembly of gemv.hip to read instead of compiling one")
    ap.add_argument("--keep", help="where to keep the compiled assembly")
    ap.add_argument("-k", "--kernel", action="append", default=[], help="substring of the demangled kernel name (repeatable)")
    ap.add_argument("--against", help="another assembly of gemv.hip: list the kernels whose body digest differs")
    ap.add_argument("--digests", action="store_true", help="print every kernel's digest")
    args = ap.parse_args()
    path = args.asm
    if not path:
        path = args.keep or os.path.join(tempfile.mkdtemp(prefix="gemv_isa_"), "gemv.s")
        compile_asm(path)
    ks = parse(path)
    pretty = demangle(sorted(ks))
    for n in sorted(ks, key=lambda n: pretty[n]):
        if any(s in pretty[n] for s in args.kernel):
            report(n, pretty[n], ks[n])
    if args.digests:
        for n in sorted(ks, key=lambda n: pretty[n]):
            print(digest(ks[n]["body"]), ks[n]["vgpr"], pretty[n])
    if args.against:
        other = parse(args.against)
        pretty.update(demangle(sorted(set(other) - set(ks))))
        same, diff = 0, []
        for n in sorted(set(ks) | set(other), key=lambda n: pretty[n]):
            if n in ks and n in other and digest(ks[n]["body"]) == digest(other[n]["body"]):
                same += 1
            else:
                diff.append(n)
        print(f"\n{len(ks)} kernels here, {len(other)} in {args.against}: {same} bodies identical, {len(diff)} not")
        for n in diff:
            side = "changed" if n in ks and n in other else ("only here" if n in ks else "only there")
            v = f"vgpr {other[n]['vgpr']} -> {ks[n]['vgpr']}" if side == "changed" else ""
            print(f"  {side:10s} {v:18s} {pretty[n]}")


if __name__ == "__main__":
    main()
