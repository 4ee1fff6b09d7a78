#!/usr/bin/env python3
"""fs2_spill_report.py -- what the compiler adds to k_train_fs2 that the resource tables do not show (CPU only, no GPU).

Compiles crux.jl_amd/csrc/train_fs2.hip to gfx950 device assembly with the Makefile's own flags (taken from `make -n train_fs2.o`) and
prints, per kernel: VGPRs, SGPRs, scratch bytes, .sgpr_spill_count, .vgpr_spill_count, code bytes, and the v_readlane_b32 / v_writelane_b32 /
s_nop counts split into "inside a minibatch loop" and "elsewhere". SGPRs spilled into VGPR lanes use no scratch, so scratch = 0 does not show them
(DESIGN 9); the lane reads and writes inside the step loop are what a step pays for them.

A minibatch loop is the depth-2 loop of a role (compute / helper waves) whose body holds v_mfma instructions, found through LLVM's loop
annotations in the assembly ("Loop Header: Depth=2", "in Loop: Header=...", "Parent Loop ..."). Where LLVM has merged a role's epoch and
minibatch loops into one depth-1 loop, that loop is taken whole (the epoch prologue and epilogue then count as inside).

  python tools/fs2_spill_report.py            # the kernels of -DCRUX_FS2_MINIMAL (the C2 / C5 learners: plain, PX, PXK, LAG, TIMING)
  python tools/fs2_spill_report.py --all      # all instantiations
  python tools/fs2_spill_report.py --json     # one JSON document instead of the table
  python tools/fs2_spill_report.py --asm F.s  # report on an assembly file made earlier (no compile)
"""
import argparse
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "crux.jl_amd", "csrc")
COUNTED = ("v_readlane_b32", "v_writelane_b32", "s_nop")
_NAME = re.compile(r"_Z11k_train_fs2ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])ELb([01])EEv9TrainArgs")
_KINDS = {0: "categorical", 1: "gaussian", 2: "value"}
_ACTS = {0: "identity", 1: "relu", 2: "tanh"}


def compile_command(all_forms):
    """the Makefile's compile line for train_fs2.o, turned into a device-assembly line (source and output are appended by the caller)"""
    line = subprocess.run(["make", "-n", "-B", "train_fs2.o"], cwd=CSRC, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
    words = shlex.split(line)
    out = []
    skip = False
    for w in words:
        if skip:
            skip = False
            continue
        if w == "-c" or w == "train_fs2.hip":
            continue
        if w == "-o":
            skip = True
            continue
        out.append(w)
    if not all_forms:
        out.append("-DCRUX_FS2_MINIMAL")
    return out + ["--cuda-device-only", "-S"]


def compile_asm(all_forms, path):
    cmd = compile_command(all_forms) + ["train_fs2.hip", "-o", path]
    r = subprocess.run(cmd, cwd=CSRC, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s\nexited with %d:\n%s" % (" ".join(cmd), r.returncode, r.stderr[-8000:]))


def describe(name):
    """(short label, dict of template arguments) of a mangled k_train_fs2 name"""
    m = _NAME.fullmatch(name)
    if not m:
        return name, {}
    i, o, kind, act, h2, act2, timing, px, pxk, lag = (int(x) for x in m.groups())
    form = "TIMING" if timing else "PXK" if pxk else "PX" if px else "LAG" if lag else "plain"
    t = {"in": i, "out": o, "kind": _KINDS.get(kind, str(kind)), "act": _ACTS.get(act, str(act)), "h2": h2, "act2": _ACTS.get(act2, str(act2)), "form": form}
    label = "%d-64-%d-%d %s %s" % (i, h2, o, t["kind"], t["act"])
    if act2 != act:
        label += "/" + t["act2"]
    return label + " " + form, t


_BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)")
_IN_LOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
_HEADER = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")
_PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=(\d+)")
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b")


def analyse_body(lines):
    """loop membership of every instruction of one kernel's body -> counts inside the minibatch loops and elsewhere"""
    parent = {}       # loop header -> its parent loop's header (or None)
    depth = {}        # loop header -> depth
    blocks = []       # (innermost loop or None, [mnemonics])
    cur_loop, cur_insns, annot = None, [], False
    label = None
    for ln in lines:
        mb = _BLOCK.match(ln)
        if mb:
            blocks.append((cur_loop, cur_insns))
            cur_loop, cur_insns, annot, label = None, [], True, mb.group(1)
        if annot and ";" in ln:
            c = ln[ln.index(";"):]
            mi = _IN_LOOP.search(c)
            if mi:
                cur_loop = mi.group(1)
            mh = _HEADER.search(c)
            if mh and label:
                cur_loop = label
                depth[label] = int(mh.group(1))
                parent.setdefault(label, None)
            mp = _PARENT.search(c)
            if mp and label:
                # the parents are listed outermost first; the last one seen before the header line is the direct parent
                parent[label] = mp.group(1)
        mi = _INSN.match(ln)
        if mi and not ln.lstrip().startswith((";", ".")):
            annot = False
            cur_insns.append(mi.group(1))
    blocks.append((cur_loop, cur_insns))

    def chain(lp):
        out = []
        while lp is not None:
            out.append(lp)
            lp = parent.get(lp)
        return out

    has_mfma = set()
    for lp, insns in blocks:
        if lp is not None and any(i.startswith("v_mfma") for i in insns):
            has_mfma.update(chain(lp))
    # one role = one top-level loop with MFMAs (its epoch loop); its minibatch loop is the depth-2 loop with the MFMAs. Where LLVM has merged the two
    # loops of a role into one (a shared header: the epoch loop then shows as Depth=1 with the spin loops as its children) that loop is taken whole,
    # epoch prologue included.
    mb_loops = []
    for top in (l for l in has_mfma if depth.get(l) == 1):
        inner = [l for l in has_mfma if depth.get(l) == 2 and chain(l)[-1] == top]
        mb_loops += inner if inner else [top]
    mb_loops.sort(key=lambda s: [int(x) for x in re.findall(r"\d+", s)])
    inside = {k: 0 for k in COUNTED}
    outside = {k: 0 for k in COUNTED}
    per_loop = {l: {k: 0 for k in COUNTED + ("instructions",)} for l in mb_loops}
    for lp, insns in blocks:
        home = next((l for l in chain(lp) if l in per_loop), None)
        for i in insns:
            if home:
                per_loop[home]["instructions"] += 1
            if i in COUNTED:
                (inside if home else outside)[i] += 1
                if home:
                    per_loop[home][i] += 1
    return {"minibatch_loops": [dict(header=l, **per_loop[l]) for l in mb_loops], "inside": inside, "elsewhere": outside}


def parse(asm_path):
    with open(asm_path) as f:
        text = f.read().splitlines()
    # metadata: one YAML list entry per kernel
    meta, cur = {}, None
    for ln in text:
        s = ln.strip()
        if s.startswith("- .agpr_count:"):
            cur = {"agpr_count": int(s.split(":")[1])}
        elif cur is not None and s.startswith(".") and ":" in s:
            k, v = s.split(":", 1)
            k, v = k.strip(" ."), v.strip()
            if k == "name":
                meta[v] = cur
            if k in ("private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "group_segment_fixed_size"):
                cur[k] = int(v)
    kernels = []
    i = 0
    while i < len(text):
        m = re.match(r"^(_Z11k_train_fs2\w+):", text[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        j = i + 1
        while j < len(text) and not text[j].startswith(".Lfunc_end"):
            j += 1
        code = None
        for k in range(j, min(j + 40, len(text))):
            mc = re.search(r"codeLenInByte = (\d+)", text[k])
            if mc:
                code = int(mc.group(1))
                break
        md = meta.get(name, {})
        label, targs = describe(name)
        row = {"name": name, "label": label, "template": targs, "vgprs": md.get("vgpr_count"), "agprs": md.get("agpr_count"), "sgprs": md.get("sgpr_count"),
               "scratch": md.get("private_segment_fixed_size"), "sgpr_spill_count": md.get("sgpr_spill_count"), "vgpr_spill_count": md.get("vgpr_spill_count"), "code_bytes": code}
        row.update(analyse_body(text[i + 1:j]))
        kernels.append(row)
        i = j
    return kernels


def table(kernels):
    hdr = "%-44s %5s %5s %7s %6s %6s %8s | %-17s | %-17s | %s" % ("kernel", "VGPR", "SGPR", "scratch", "s.spl", "v.spl", "code B", "loops rd/wr/nop", "elsewhere rd/wr/nop", "per minibatch loop: insns rd wr nop")
    out = [hdr, "-" * len(hdr)]
    for k in sorted(kernels, key=lambda r: (r["template"].get("in", 0), r["template"].get("h2", 0), r["template"].get("out", 0), r["label"])):
        ins, oth = k["inside"], k["elsewhere"]
        loops = "  ".join("%d %d %d %d" % (l["instructions"], l["v_readlane_b32"], l["v_writelane_b32"], l["s_nop"]) for l in k["minibatch_loops"])
        out.append("%-44s %5s %5s %7s %6s %6s %8s | %5d %5d %5d | %5d %5d %5d   | %s" % (k["label"], k["vgprs"], k["sgprs"], k["scratch"], k["sgpr_spill_count"], k["vgpr_spill_count"], k["code_bytes"],
                                                                                    ins["v_readlane_b32"], ins["v_writelane_b32"], ins["s_nop"], oth["v_readlane_b32"], oth["v_writelane_b32"], oth["s_nop"], loops))
    return "\n".join(out)


def report(all_forms=False, asm=None):
    if asm:
        return parse(asm)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "train_fs2.s")
        compile_asm(all_forms, path)
        return parse(path)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--all", action="store_true", help="every instantiation (minutes), not only those of -DCRUX_FS2_MINIMAL")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--asm", help="an assembly file made earlier")
    a = ap.parse_args()
    ks = report(a.all, a.asm)
    print(json.dumps(ks, indent=1) if a.json else table(ks))
    return 0


if __name__ == "__main__":
    sys.exit(main())
