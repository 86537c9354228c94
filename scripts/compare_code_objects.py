"""Compare the gfx950 device code of two builds of libfa2_amd.so, kernel by kernel.

usage: python scripts/compare_code_objects.py A.so B.so [--allow SYMBOL_SUBSTRING ...] [-q]

For a change that must not touch device code (a host-side refactor): build the parent and the
branch into separate FA2_BUILD_DIR / FA2_LIB_OUT and run this on the two libraries.  Per function
symbol of the gfx950 code objects it prints `bytes equal`, `bytes differ`, `only in A` or `only in
B` (-q: only the ones that are not equal), per kernel descriptor whether (scratch, VGPRs, LDS) are equal, then
one summary line.  Exit status 1 on any difference whose symbol contains none of the --allow
substrings.  Only bytes and descriptor fields are compared (descriptor code-entry offsets may move).
A symbol instantiated in several translation units is compared as the set of its distinct versions.
"""
import argparse
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_code_objects import _code_objects, _kernel_descriptors, _sections  # noqa: E402

STT_FUNC = 2


def _functions(co: bytes):
    """{function symbol: its bytes} of one code object."""
    secs, heads = _sections(co)
    name, typ, addr, off, size, link, entsize = secs[".symtab"] if ".symtab" in secs else secs[".dynsym"]
    stroff = heads[link][3]
    out = {}
    for i in range(size // 24):
        st_name, st_info, st_other, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", co, off + i * 24)
        if st_info & 0xF != STT_FUNC or st_shndx == 0 or st_shndx >= len(heads):
            continue
        sym = co[stroff + st_name: co.index(b"\0", stroff + st_name)].decode()
        sh = heads[st_shndx]
        fo = sh[3] + (st_value - sh[2])
        out[sym] = co[fo: fo + st_size]
    return out


def read_library(path):
    funcs, descs = {}, {}
    for co in _code_objects(path):
        for sym, code in _functions(co).items():
            funcs.setdefault(sym, set()).add(code)
        for sym, fields in _kernel_descriptors(co).items():
            descs.setdefault(sym, set()).add(fields)
    return funcs, descs


def compare(a, b, label, quiet):
    """Prints one line per symbol; returns {symbol: verdict} of those that are not equal."""
    bad = {}
    for sym in sorted(set(a) | set(b)):
        verdict = "only in A" if sym not in b else "only in B" if sym not in a else \
            f"{label} equal" if a[sym] == b[sym] else f"{label} differ"
        if not verdict.endswith("equal"):
            bad[sym] = verdict
        if not quiet or sym in bad:
            print(f"{verdict}: {sym}")
    return bad


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--allow", action="append", default=[], metavar="SYMBOL_SUBSTRING")
    ap.add_argument("-q", action="store_true", help="do not print the equal symbols")
    args = ap.parse_args(argv)
    (fa, da), (fb, db) = read_library(args.a), read_library(args.b)
    bad_f = compare(fa, fb, "bytes", args.q)
    bad_d = compare(da, db, "(scratch, VGPRs, LDS)", args.q)
    refused = [s for s in list(bad_f) + list(bad_d) if not any(sub in s for sub in args.allow)]
    print(f"{len(set(fa) | set(fb))} functions, {len(bad_f)} differ or are missing; {len(set(da) | set(db))} kernel "
          f"descriptors, {len(bad_d)} differ or are missing; {len(refused)} of these not allowed")
    return 1 if refused else 0


if __name__ == "__main__":
    sys.exit(main())
