#!/usr/bin/env python3
"""Static ISA census of every product kernel -> profiles/isa_<source hash>.json.

Compiles the record kernels' HIP sources with the product flags and --save-temps (CPU
only, hipcc cross-compiles gfx950), then runs tools/isa_count.py's census on
each kernel: its record loop (the body between the loop header and its
back-edge) for the persistent kernels, otherwise the whole function.  Per
kernel (rocprofv3's demangled name):

  arx_full / arx_rot   VALU inside the generated double-round asm
                       (v_add/v_xor pair at 2 clocks in lock-step, v_alignbit
                       at 4: profiles/r01_valu_issue_probes.md)
  other_valu           every other VALU of the census (static, all paths),
                       split into other_full (full-rate opcodes: add, xor,
                       and, or, mov, right shifts, bitop3) and other_half
  mfma, lds, vmem, salu
  skeleton             a hash of the kernel's ordered memory, wait, barrier and
                       MFMA opcodes (isa_count.skeleton)
  clk_per_valu         the issue model's clocks per VALU instruction of this
                       mix: full-rate opcodes 2 (paired with the SIMD's other
                       lock-step wave, as the FF A/B of profiles/r04_ab shows
                       outside the asm too), every other VALU 4

bench.py prices the PMC-counted dynamic VALU of a launch with clk_per_valu
(valu_roofline), and DESIGN.md §4.2's ISA table is this file's C1 entry.
Usage: python tools/isa_census.py [--keep DIR] [--against profiles/isa_<parent hash>.json]

--against compares this tree's census with an earlier one and writes only the
comparison, profiles/isa_<hash>_vs_<parent hash>.json: how many of the parent's
entries are identical in every field, those that changed with the names of
the fields that differ, those that are gone, and every new kernel with its registers, VALU, LDS and scratch (the whole
census of a tree with every record form is some 16,000 lines).
"""
from __future__ import annotations

import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import isa_count as ic  # noqa: E402

from suruga_amd import _build  # noqa: E402

FULL = ic.FULL
DRAFT_ARG = ", (sg::Construction)0"  # Construction::kDraft as c++filt prints it
# The record kernels that take the TLS 1.3 record form as their last template argument
# (T13 / TLS13, a bool): "..., false>(" is the form they had before it.
T13_KERNELS = ("sg_wpr_kernel<", "sg_wpr_keying_kernel<", "sg_aead_kernel<", "sg_aead_list_kernel<", "sg_keying_kernel<",
               "sg_classify_kernel<", "sg_pack_kernel<")
T13_OFF = ", false>("


# every file of the library that holds a kernel (one that the tree does not have yet is passed over, so
# that the tool can take the census of an earlier commit)
SOURCES = [_build.CSRC / f for f in ("sg_wpr.hip", "sg_wpr_keying.hip", "sg_pack.hip", "sg_kernels.hip", "sg_plumb.hip",
                                     "sg_msg.hip", "sg_msg_batch.hip", "sg_quic.hip", "sg_wg.hip", "sg_esp.hip", "sg_dtls13.hip", "sg_hkdf.hip")
           if (_build.CSRC / f).exists()]


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return p.stdout.splitlines()


def census_file(path: Path):
    lines = path.read_text().splitlines()
    names = [l[:-1].split(":")[0] for l in lines if l.startswith("_Z") and l.rstrip().endswith(":") is False
             and ":" in l and "sg_" in l.split(":")[0]]
    names = []
    for l in lines:
        if l.startswith("_Z") and ":" in l:
            nm = l.split(":")[0]
            if "_kernel" in nm and nm not in names:
                names.append(nm)
    # the code object's own metadata: registers, LDS and scratch per kernel
    # (amdhsa.kernels: one "  - .key: value" entry per kernel, keys in alphabetical order)
    res, cur = {}, None
    for l in lines:
        if re.match(r"  - \.", l):
            cur = {}
        m = re.match(r"  [ -] \.(group_segment_fixed_size|private_segment_fixed_size|sgpr_count|vgpr_count|name):\s+(\S+)", l)
        if m and cur is not None:
            if m.group(1) == "name":
                res[m.group(2)] = cur
            else:
                cur[m.group(1)] = int(m.group(2))
    out = {}
    for mangled, dem in zip(names, demangle(names)):
        body_all = ic.kernel_lines(str(path), mangled)
        body = ic.loop_body(body_all)
        looped = len(body) != len(body_all)
        arx, other, kinds, _ = ic.census(body)
        af = sum(v for k, v in arx.items() if k in FULL)
        ar = sum(arx.values()) - af
        oth = sum(other.values())
        oth_full = sum(v for k, v in other.items() if k.split("_e32")[0].split("_e64")[0] in FULL)
        tot = af + ar + oth
        out[dem] = {"scope": "record loop" if looped else "whole kernel", "arx_full": af, "arx_rot": ar,
                    "other_valu": oth, "other_full": oth_full, "other_half": oth - oth_full, "valu": tot,
                    "mfma": kinds.get("mfma", 0), "lds": kinds.get("lds", 0),
                    "vmem": kinds.get("vmem", 0), "salu": kinds.get("salu", 0),
                    "clk_per_valu": round((2 * (af + oth_full) + 4 * (ar + oth - oth_full)) / tot, 4) if tot else None,
                    "other_by_op": dict(other.most_common(16))}
        # the whole function's mix (setup and tails included): what bench.py
        # prices a kernel's PMC-counted VALU with (a loop region of a kernel
        # with a complex CFG need not hold all of its per-iteration code)
        warx, woth, _, _ = ic.census(body_all)
        waf = sum(v for k, v in warx.items() if k in FULL)
        war = sum(warx.values()) - waf
        wof = sum(v for k, v in woth.items() if k.split("_e32")[0].split("_e64")[0] in FULL)
        wtot = waf + war + sum(woth.values())
        out[dem]["whole"] = {"arx_full": waf, "arx_rot": war, "other_full": wof,
                             "other_half": sum(woth.values()) - wof, "valu": wtot}
        out[dem]["resources"] = res.get(mangled, {})
        out[dem]["skeleton"] = ic.skeleton(body_all)  # the order its counted waits and barriers depend on
        out[dem]["clk_per_valu_whole"] =round((2 * (waf + wof) + 4 * (wtot - waf - wof)) / wtot, 4) if wtot else None
    return out


def compare(parent: dict, kernels: dict) -> dict:
    """This tree's census entries against an earlier census's, entry by entry."""
    def row(v):
        r = v["resources"]
        return {"vgpr": r.get("vgpr_count"), "sgpr": r.get("sgpr_count"), "valu": v["whole"]["valu"], "mfma": v["mfma"],
                "lds_bytes": r.get("group_segment_fixed_size"), "scratch_bytes": r.get("private_segment_fixed_size")}

    def fields(k):  # the fields of k that differ (a census from before the skeleton field: compared without it)
        new = kernels[k] if "skeleton" in parent[k] else {f: v for f, v in kernels[k].items() if f != "skeleton"}
        return sorted(f for f in set(new) | set(parent[k]) if new.get(f) != parent[k].get(f))

    return {"parent_entries": len(parent), "identical": sum(1 for k in parent if k in kernels and not fields(k)),
            "changed": {k: fields(k) for k in sorted(parent) if k in kernels and fields(k)},
            "missing": sorted(k for k in parent if k not in kernels),
            # a kernel that only gained a template argument is its parent's entry under a longer name
            "renamed": sum(1 for k in kernels if k not in parent and T13_OFF in k and k.replace(T13_OFF, ">(") in parent),
            "new": {k: row(kernels[k]) for k in kernels
                    if k not in parent and not (T13_OFF in k and k.replace(T13_OFF, ">(") in parent)}}


def dump_compact(cmp: dict) -> str:
    """JSON with one changed and one new kernel per line."""
    head = {k: v for k, v in cmp.items() if k not in ("changed", "new")}
    rows = {f: ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in cmp[f].items()) for f in ("changed", "new")}
    return (json.dumps(head, indent=1)[:-2] + ',\n "changed": {\n' + rows["changed"] + '\n },\n "new": {\n' + rows["new"]
            + "\n }\n}\n")


def main():
    against = Path(sys.argv[sys.argv.index("--against") + 1]) if "--against" in sys.argv else None
    keep = None
    if "--keep" in sys.argv:
        keep = Path(sys.argv[sys.argv.index("--keep") + 1])
        keep.mkdir(parents=True, exist_ok=True)
    src = _build.source_hash()
    with tempfile.TemporaryDirectory(prefix="sg_isa_") as td:
        wd = keep or Path(td)
        kernels = {}
        for s in SOURCES:
            flags = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-mllvm",
                     "-amdgpu-atomic-optimizer-strategy=None", "--save-temps", f'-DSG_SOURCE_HASH="{src}"']
            subprocess.run([_build.hipcc(), *flags, "-c", "-o", str(wd / f"{s.stem}.o"), str(s)], cwd=wd, check=True,
                           capture_output=True)
            kernels.update(census_file(wd / f"{s.stem}-hip-amdgcn-amd-amdhsa-gfx950.s"))
    res = {"source_hash": src, "model": "clocks per wave64 VALU: full-rate opcodes (v_add/v_xor/v_and/v_or/v_mov/"
                                        "right shifts/bitop3) 2, paired in lock-step; rotates and every other VALU 4 "
                                        "(profiles/r01_valu_issue_probes.md)",
           "kernels": kernels}
    # The draft instantiations of the record kernels that take the construction as a
    # template parameter (Construction, sg_layout.h) are also listed under the name they
    # had before the parameter: bench.py's C1 roofline and earlier profiles look the
    # draft kernel up by that name, and it is the same kernel.
    # (The message kernels share the parameter and were never looked up by a
    # shorter name: they keep their one entry.)
    # Likewise the instantiations without the TLS 1.3 record form, which are the kernels
    # of before that argument: listed under the name without it as well (first, so
    # that a draft kernel also gets its shortest name).
    for k in list(kernels):
        if T13_OFF in k and any(f in k for f in T13_KERNELS):
            kernels.setdefault(k.replace(T13_OFF, ">("), kernels[k])
    for k in list(kernels):
        if DRAFT_ARG in k and "sg_msg" not in k:
            kernels.setdefault(k.replace(DRAFT_ARG, ""), kernels[k])
    if against is not None:
        old = json.loads(against.read_text())
        cmp = {"source_hash": src, "parent_source_hash": old["source_hash"], **compare(old["kernels"], kernels)}
        dst = ROOT / "profiles" / f"isa_{src}_vs_{old['source_hash']}.json"
        dst.write_text(dump_compact(cmp))
        print(dst, cmp["identical"], "of", cmp["parent_entries"], "identical,", len(cmp["new"]), "new")
        return
    dst = ROOT / "profiles" / f"isa_{src}.json"
    dst.write_text(json.dumps(res, indent=1) + "\n")
    print(dst)
    for k, v in kernels.items():
        if "wpr_kernel<false, true, 4u, false" in k or "wpr_kernel<true, true, 4u, false" in k:
            print(k, {x: v[x] for x in ("arx_full", "arx_rot", "other_full", "other_half", "mfma", "clk_per_valu")})


if __name__ == "__main__":
    main()
