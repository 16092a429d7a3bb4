#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds the same?  Per kernel symbol: a hash of its .text bytes and its
resource notes (VGPRs, SGPRs, AGPRs, scratch, LDS, kernarg size).

    tools/kernel_identity.py BUILD_A BUILD_B [--json OUT]
    tools/kernel_identity.py --a a/*.o --b b/*.o [--json OUT]

BUILD_A / BUILD_B are build directories of csrc/Makefile (csrc/_build): their ikpso_inst_*.hip.o and
ikpso_kernels.hip.o are compared unit by unit.  With --a / --b the objects are listed (host objects as
the Makefile builds them, or `hipcc --cuda-device-only -c` outputs with the Makefile's flags) and paired
by file name.  Prints the kernel symbols added, removed and changed, writes a JSON summary, and exits 1
if anything differs.  CPU only: clang-offload-bundler and llvm-readelf of the ROCm install ($ROCM_PATH,
default /opt/rocm) read the objects; nothing is disassembled.
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
NOTES = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
         "kernarg_segment_size", "uses_dynamic_stack")
BUNDLE_MAGICS = (b"__CLANG_OFFLOAD_BUNDLE__", b"CCOB")


def tool(name, *args):
    return subprocess.run([str(LLVM / name), *args], check=True, capture_output=True, text=True).stdout


def sections(path):
    """{name: (index, address, file offset, size)} of an ELF file."""
    out = {}
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)",
                         tool("llvm-readelf", "-S", "--wide", str(path)), re.M):
        out[m.group(2)] = (int(m.group(1)), int(m.group(3), 16), int(m.group(4), 16), int(m.group(5), 16))
    return out


def code_object(path, tmp):
    """The gfx950 code object of `path`: a host object with the bundle in .hip_fatbin, a bundle, or the
    code object itself."""
    data = Path(path).read_bytes()
    bundle = None
    if data.startswith(BUNDLE_MAGICS):
        bundle = data
    elif data[:4] == b"\x7fELF" and int.from_bytes(data[18:20], "little") != 224:  # not EM_AMDGPU: a host object
        _, _, off, size = sections(path)[".hip_fatbin"]
        bundle = data[off:off + size]
    if bundle is None:
        return Path(path)
    src, dst = Path(tmp) / "bundle", Path(tmp) / (Path(path).name + ".co")
    src.write_bytes(bundle)
    tool("clang-offload-bundler", "--type=o", "--unbundle", f"--targets={TARGET}", f"--input={src}", f"--output={dst}")
    return dst


def kernel_notes(co):
    """{kernel name: {note: value}} from the code object's amdhsa.kernels metadata."""
    kernels, cur, indent = {}, None, None
    for line in tool("llvm-readelf", "--notes", str(co)).splitlines():
        m = re.match(r"^(\s*)(- )?\.(\w+):\s*(.*)$", line)
        if line.startswith("amdhsa.kernels:"):
            indent = -1
            continue
        if indent is None or not m:
            if indent is not None and re.match(r"^amdhsa\.\w+:", line):
                indent = None  # the kernels' list is over
            continue
        depth = len(m.group(1)) + (2 if m.group(2) else 0)
        if indent == -1:
            indent = depth
        if depth != indent:
            continue  # a kernel's arguments
        if m.group(2):
            cur = {}
        if m.group(3) == "name":
            kernels[m.group(4).strip("'\"")] = cur
        elif m.group(3) in NOTES:
            cur[m.group(3)] = m.group(4)
    return kernels


def kernels_of(path, tmp):
    """{kernel symbol: {"text": sha256 of its bytes, "size": n, notes...}} of one object."""
    co = code_object(path, tmp)
    data = co.read_bytes()
    by_index = {idx: (addr, off) for idx, addr, off, _ in sections(co).values()}
    funcs, descriptors = {}, set()
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(\w+)\s+\w+\s+\w+\s+(\d+)\s+(\S+)",
                         tool("llvm-readelf", "--symbols", "--wide", str(co)), re.M):
        value, size, kind, shndx, name = int(m.group(1), 16), int(m.group(2)), m.group(3), int(m.group(4)), m.group(5)
        if kind == "FUNC":
            funcs[name] = (value, size, shndx)
        elif name.endswith(".kd"):
            descriptors.add(name[:-3])
    notes = kernel_notes(co)
    out = {}
    for name in sorted(descriptors):
        value, size, shndx = funcs[name]
        addr, off = by_index[shndx]
        text = data[off + value - addr:off + value - addr + size]
        out[name] = dict(text=hashlib.sha256(text).hexdigest(), size=size, **notes.get(name, {}))
    return out


def units_of(spec):
    """{unit name: object path} of a build directory or a list of objects."""
    if len(spec) == 1 and Path(spec[0]).is_dir():
        d = Path(spec[0])
        spec = sorted(d.glob("ikpso_inst_*.hip.o")) + [d / "ikpso_kernels.hip.o"]
    return {Path(p).name: Path(p) for p in spec}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("builds", nargs="*", help="two build directories")
    ap.add_argument("--a", nargs="+", help="objects of the first build")
    ap.add_argument("--b", nargs="+", help="objects of the second build")
    ap.add_argument("--json", default=None, help="write the summary here")
    args = ap.parse_args()
    if args.a and args.b:
        a, b = units_of(args.a), units_of(args.b)
    elif len(args.builds) == 2:
        a, b = units_of(args.builds[:1]), units_of(args.builds[1:])
    else:
        ap.error("give two build directories, or --a and --b")
    summary = dict(units=0, kernels=0, identical=0, added=[], removed=[], changed=[], units_only_in_a=sorted(set(a) - set(b)),
                   units_only_in_b=sorted(set(b) - set(a)), per_unit={})
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        for unit in sorted(set(a) & set(b)):
            ka, kb = kernels_of(a[unit], ta), kernels_of(b[unit], tb)
            added, removed = sorted(set(kb) - set(ka)), sorted(set(ka) - set(kb))
            changed = {k: sorted(f for f in set(ka[k]) | set(kb[k]) if ka[k].get(f) != kb[k].get(f))
                       for k in sorted(set(ka) & set(kb)) if ka[k] != kb[k]}
            same = len(set(ka) & set(kb)) - len(changed)
            digest = hashlib.sha256("".join(k + kb[k]["text"] for k in sorted(kb)).encode()).hexdigest()[:16]
            summary["per_unit"][unit] = dict(kernels=len(kb), identical=same, added=len(added), removed=len(removed),
                                             changed=len(changed), digest=digest)
            summary["units"] += 1
            summary["kernels"] += len(kb)
            summary["identical"] += same
            summary["added"] += [f"{unit}: {k}" for k in added]
            summary["removed"] += [f"{unit}: {k}" for k in removed]
            summary["changed"] += [f"{unit}: {k} ({', '.join(f)})" for k, f in changed.items()]
    for what in ("added", "removed", "changed", "units_only_in_a", "units_only_in_b"):
        for line in summary[what]:
            print(f"{what}: {line}")
    print(f"{summary['units']} units, {summary['kernels']} kernels: {summary['identical']} identical, "
          f"{len(summary['added'])} added, {len(summary['removed'])} removed, {len(summary['changed'])} changed")
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(summary, indent=1, sort_keys=True) + "\n")
    different = any(summary[w] for w in ("added", "removed", "changed", "units_only_in_a", "units_only_in_b"))
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
