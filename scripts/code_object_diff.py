"""Compare the gfx950 code objects of two builds of the library, one line per translation unit.

    python scripts/code_object_diff.py PARENT/libteal_hip.so TREE/libteal_hip.so [--label product]

Each library is taken apart the way tests/test_host_logic.py::test_no_packed_fp32_instruction_in_the_libraries does it
(`llvm-objdump --offloading`: one code object per translation unit, in link order = teal_amd._lib.SOURCES).  The TEXT of a code
object is its symbol table and disassembly (`llvm-objdump -t -d`) followed by its metadata notes (`llvm-readelf --notes`: the
register, LDS, scratch and spill figures of every kernel).  `compare(parent_text, tree_text)` is a pure function of two such
texts and says

    identical   every line is the parent's (the file-name header and the __hip_cuid_* object — a hash of the source — aside)
    renamed     for every symbol the sequence of mnemonics is the parent's, every kernel's figures are the parent's and the
                symbol set is the parent's: only operands (register numbers, the order of commutative sources) differ
    different   anything else

It is a generic comparison: it looks for no particular instruction.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
CUID = "__hip_cuid_"
# per-kernel figures of the metadata notes that a renaming must leave alone
FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
           ".vgpr_spill_count", ".sgpr_spill_count")

_LABEL = re.compile(r"^[0-9a-fA-F]+ <([^>]+)>:\s*$")
_SYMBOL = re.compile(r"^[0-9a-fA-F]+\s+\w?\s+\w*\s*[FO]\s+\S+\s+[0-9a-fA-F]+\s+(?:\.\w+\s+)?(\S+)\s*$")
_FIGURE = re.compile(r"^\s*-?\s*(\.[a-z_]+):\s*(\S+)\s*$")


def _lines(text: str):
    """The lines that are compared: no blank line, no file-name header, nothing that names the source hash object."""
    return [ln.rstrip() for ln in text.splitlines() if ln.strip() and "file format" not in ln and CUID not in ln]


def _mnemonics(lines):
    """{symbol: [mnemonic, ...]} of the disassembly lines (an instruction line is `<tab>mnemonic operands // address: encoding`)."""
    out, cur = {}, None
    for ln in lines:
        m = _LABEL.match(ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and ln[:1] in ("\t", " ") and "//" in ln:
            cur.append(ln.split("//")[0].split()[0])
    return out


def _symbols(lines):
    """Defined function / object symbols of the symbol table."""
    return {m.group(1) for m in map(_SYMBOL.match, lines) if m}


def _figures(lines):
    """{kernel descriptor: {figure: value}} of the metadata notes.  A kernel's entry holds `.symbol:` (only kernels have one)
    and each figure once, so a key that comes again opens the next entry."""
    out, entry = {}, {}
    for ln in lines + ["    .symbol: end"]:
        m = _FIGURE.match(ln)
        if not m or not (m.group(1) == ".symbol" or m.group(1) in FIGURES):
            continue
        if m.group(1) in entry:
            out[entry.get(".symbol", "?")] = {k: entry.get(k) for k in FIGURES}
            entry = {}
        entry[m.group(1)] = m.group(2)
    if len(entry) > 1:
        out[entry.get(".symbol", "?")] = {k: entry.get(k) for k in FIGURES}
    return out


def compare(parent_text: str, tree_text: str) -> dict:
    """{"verdict": identical | renamed | different, "lines": compared lines of the tree, "differing": lines that differ,
    "symbols": symbols compared, "why": what made it `different` (empty otherwise)}"""
    a, b = _lines(parent_text), _lines(tree_text)
    sa, sb = _symbols(a), _symbols(b)
    res = {"lines": len(b), "differing": 0, "symbols": len(sb), "why": ""}
    if a == b:
        return {**res, "verdict": "identical"}
    res["differing"] = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
    ma, mb = _mnemonics(a), _mnemonics(b)
    if sa != sb or set(ma) != set(mb):
        odd = sorted((sa ^ sb) | (set(ma) ^ set(mb)))
        return {**res, "verdict": "different", "why": f"symbol set: {odd[0]} (+{len(odd) - 1})"}
    for name in ma:
        if ma[name] != mb[name]:
            at = next((i for i, (x, y) in enumerate(zip(ma[name], mb[name])) if x != y), min(len(ma[name]), len(mb[name])))
            return {**res, "verdict": "different", "why": f"mnemonics of {name} at instruction {at}"}
    fa, fb = _figures(a), _figures(b)
    if fa != fb:
        odd = sorted(k for k in set(fa) | set(fb) if fa.get(k) != fb.get(k))
        return {**res, "verdict": "different", "why": f"figures of {odd[0]}"}
    return {**res, "verdict": "renamed"}


def unit_texts(lib: str, workdir: str):
    """The text of every gfx950 code object of `lib`, in link order."""
    os.makedirs(workdir)
    shutil.copy(lib, os.path.join(workdir, "lib.so"))
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=workdir, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    objs = [f for f in os.listdir(workdir) if f.endswith("gfx950")]
    objs.sort(key=lambda f: int(re.search(r"[.:](\d+)\.hip", f).group(1)))
    for f in objs:
        yield (subprocess.check_output([OBJDUMP, "-t", "-d", f], cwd=workdir, text=True)
               + subprocess.check_output([READELF, "--notes", f], cwd=workdir, text=True))


def table(parent_lib: str, tree_lib: str, label: str, sources) -> list:
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        pa, tr = list(unit_texts(parent_lib, os.path.join(tmp, "parent"))), list(unit_texts(tree_lib, os.path.join(tmp, "tree")))
    # (a tree may append translation units to SOURCES: the parent's units are compared, the new ones are listed as `new`)
    if not (len(pa) <= len(tr) == len(sources)):
        raise SystemExit(f"{len(pa)} / {len(tr)} code objects for {len(sources)} translation units")
    for src, t in zip(sources[len(pa):], tr[len(pa):]):
        sha = hashlib.sha256("\n".join(_lines(t)).encode()).hexdigest()[:16]
        rows.append(f"  {label:<12} {src:<30} {len(_lines(t)):>7} lines {len(_symbols(_lines(t))):>5} symbols  {'new':<9}  sha256 {sha}")
    for src, p, t in zip(sources, pa, tr):
        r = compare(p, t)
        sha = hashlib.sha256("\n".join(_lines(t)).encode()).hexdigest()[:16]
        tail = f"  {r['differing']} lines differ" if r["verdict"] != "identical" else ""
        rows.append(f"  {label:<12} {src:<30} {r['lines']:>7} lines {r['symbols']:>5} symbols  {r['verdict']:<9}  sha256 {sha}{tail}"
                    + (f"  ({r['why']})" if r["why"] else ""))
    return rows


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent_lib")
    ap.add_argument("tree_lib")
    ap.add_argument("--label", default="product")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from teal_amd._lib import SOURCES
    rows = table(args.parent_lib, args.tree_lib, args.label, SOURCES)
    print("\n".join(rows))
    return 0 if all(" different " not in r for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
