#!/usr/bin/env python3
"""Wait map of the kernels of one HIP source: compiles csrc/<file>.hip to gfx950 assembly with the Makefile's flags (no GPU needed) and prints,
per kernel, the order in which the instruction stream issues vector-memory loads, LDS-DMA loads, stores, `s_waitcnt vmcnt(N)`, barriers and
MFMA runs -- what the pipelining written in the source has become -- with VGPRs, scratch and occupancy.

    L      global / buffer / flat / scratch load into registers        G   load straight into LDS (`... lds`)
    S      store                                                       A   vector-memory atomic
    W(n)   s_waitcnt with vmcnt(n)                                     B   s_barrier
    M*k    a run of k MFMAs (other ALU / LDS instructions do not break a run)
    br     a forward s_cbranch_execz / vccz / scc: what follows may be skipped, so hipcc cannot count it (a later wait for anything older is W(0))
    <      a backward branch (a loop: the sequence since its label repeats)
Repeats are folded: `Lx9`, `[br L]x10`.  The order is that of the assembly text: a block hipcc has placed out of line shows where it stands.

usage: python tools/kernel_wait_map.py <file.hip | file.s> [<kernel-name substring> ...] [--arch gfx950] [--raw]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "computervision_codes_amd", "csrc")


def makefile_flags(arch):
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"):
            flags = line.split("=", 1)[1].split()
    if flags is None:
        sys.exit("no CXXFLAGS in the Makefile")
    return [f.replace("$(ARCH)", arch) for f in flags]


def compile_to_asm(src, arch):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + makefile_flags(arch) + ["--cuda-device-only", "-S", os.path.basename(src), "-o", out]
    subprocess.run(cmd, cwd=os.path.dirname(os.path.abspath(src)), check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    os.unlink(out)
    return text


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


LOAD = re.compile(r"^(global|buffer|flat|scratch)_load_")
STORE = re.compile(r"^(global|buffer|flat|scratch)_store_")
ATOMIC = re.compile(r"^(global|buffer|flat)_atomic_")
VMCNT = re.compile(r"vmcnt\((\d+)\)")
LABEL = re.compile(r"^([.\w$]+):")
BRANCH = re.compile(r"^s_cbranch_(\w+)\s+([.\w$]+)")


def events(body):
    """tokens of one kernel body (a list of assembly lines)"""
    ev, seen, mfma = [], set(), 0

    def flush():
        nonlocal mfma
        if mfma:
            ev.append(f"M*{mfma}")
            mfma = 0

    for raw in body:
        line = raw.split(";")[0].strip()
        if not line:
            continue
        m = LABEL.match(line)
        if m:
            seen.add(m.group(1))
            continue
        op = line.split()[0]
        if op.startswith("v_mfma") or op.startswith("v_smfma"):
            mfma += 1
            continue
        tok = None
        if LOAD.match(op):
            tok = "G" if re.search(r"\blds\b", line) else "L"
        elif STORE.match(op):
            tok = "S"
        elif ATOMIC.match(op):
            tok = "A"
        elif op == "s_barrier":
            tok = "B"
        elif op == "s_waitcnt":
            w = VMCNT.search(line)
            if w:
                tok = f"W({w.group(1)})"
        else:
            b = BRANCH.match(line)
            if b:
                tok = "<" if b.group(2) in seen else "br"
            elif op == "s_branch" and line.split()[1] in seen:
                tok = "<"
        if tok:
            flush()
            ev.append(tok)
    flush()
    return ev


def fold(ev):
    """[br, L, br, L, L, L] -> '[br L]x2 Lx2': at each position the repeating group (up to 8 tokens) that covers most, the shorter on a tie"""
    out, i = [], 0
    while i < len(ev):
        best_g, best_n = 1, 1
        for g in range(1, 9):
            n = 1
            while ev[i + g * n:i + g * (n + 1)] == ev[i:i + g]:
                n += 1
            if n > 1 and g * n > best_g * best_n:
                best_g, best_n = g, n
        grp = ev[i:i + best_g]
        if best_g == 1 and grp[0] == "br" and best_n == 1 and i + 1 < len(ev) and ev[i + 1] in ("L", "S", "G"):
            out.append(f"[br {ev[i + 1]}]")              # a lone conditional load / store reads better bracketed
            i += 2
            continue
        txt = grp[0] if best_g == 1 else "[" + (" ".join(grp) if best_g == 2 else fold(grp)) + "]"
        out.append(txt + (f"x{best_n}" if best_n > 1 else ""))
        i += best_g * best_n
    return " ".join(out)


def kernels(text):
    """(name, body lines, {metadata}) of every kernel in an assembly file"""
    lines = text.split("\n")
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    res = []
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))    # not the first s_endpgm: blocks may follow it
        meta = {}
        for ln in lines[end:end + 400]:
            m = re.match(r";\s*(NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", ln.strip())
            if m and m.group(1) not in meta:
                meta[m.group(1)] = int(m.group(2))
        res.append((name, lines[start + 1:end], meta))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source")
    ap.add_argument("substr", nargs="*")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--raw", action="store_true", help="one token per instruction, unfolded")
    a = ap.parse_args()
    src = a.source if os.path.exists(a.source) else os.path.join(CSRC, a.source)
    text = open(src).read() if src.endswith(".s") else compile_to_asm(src, a.arch)
    ks = kernels(text)
    pretty = demangle([k[0] for k in ks])
    print(f"# {os.path.basename(src)}  ({a.arch})")
    for name, body, meta in ks:
        shown = pretty[name].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if a.substr and not any(s in shown or s in name for s in a.substr):
            continue
        ev = events(body)
        print(f"\n{shown}")
        print(f"  VGPRs {meta.get('NumVgprs', '?')} + AGPRs {meta.get('NumAgprs', '?')}, scratch {meta.get('ScratchSize', '?')} B, "
              f"occupancy {meta.get('Occupancy', '?')} waves/SIMD, static LDS {meta.get('LDSByteSize', '?')} B")
        print("  " + (" ".join(ev) if a.raw else fold(ev)))


if __name__ == "__main__":
    main()
