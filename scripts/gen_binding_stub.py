"""Generates the ctypes binding stub of INTEGRATION.md section 2 from include/gode.h, so the document cannot drift
from the header: every `typedef struct` becomes a ctypes.Structure with the same fields in the same order, every
`GODE_OP_*` kind of the header's GODE_OPS table is listed with its struct and its entry point gets its prototype, and the
stub checks itself against gode_sizeof() when executed.

  python scripts/gen_binding_stub.py            # prints the stub
  python scripts/gen_binding_stub.py --write    # rewrites the block between the markers in INTEGRATION.md

tests/test_integration_doc.py asserts that the committed block equals this output and executes it.
"""
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gode.h")
DOC = os.path.join(REPO, "INTEGRATION.md")
BEGIN, END = "<!-- BEGIN GENERATED BINDING STUB (scripts/gen_binding_stub.py) -->", "<!-- END GENERATED BINDING STUB -->"

SCALARS = {"int32_t": "i32", "int64_t": "i64", "float": "f32", "int": "C.c_int"}


def parse_structs(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        name, body = m.group(3), m.group(2)
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            mm = re.match(r"^(const\s+)?(\w+)\s*(\*?)\s*(.*)$", decl)
            base, star, rest = mm.group(2), mm.group(3), mm.group(4)
            for d in rest.split(","):
                d = d.strip()
                ptr = bool(star) or d.startswith("*")
                d = d.lstrip("* ")
                arr = re.match(r"^(\w+)\[(\d+)\]$", d)
                if ptr:
                    ctype = "ptr"
                elif base in SCALARS:
                    ctype = SCALARS[base]
                else:
                    ctype = base          # nested struct, declared earlier in the header
                if arr:
                    fields.append((arr.group(1), f"{ctype} * {arr.group(2)}"))
                else:
                    fields.append((d, ctype))
        out.append((name, fields))
    return out


def parse_ops(text):
    """The rows of the header's GODE_OPS table: (NAME, value, op struct, entry point)."""
    table = re.search(r"#define\s+GODE_OPS\(X\)(.*?[^\\])\n", text, flags=re.S).group(1)
    return [(n, int(v), st, fn) for n, v, st, fn in re.findall(r"X\(\s*(\w+)\s*,\s*(\d+)\s*,\s*(\w+)\s*,\s*(\w+)\s*\)", table)]


def parse_kinds(text):
    """Every GODE_OP_* kind with its struct, in numeric order: the table rows plus PACK, which the header keeps out of the
    table (it has no entry point of the common form)."""
    pack = int(re.search(r"GODE_OP_PACK\s*=\s*(\d+)", text).group(1))
    return sorted([(v, st) for _, v, st, _ in parse_ops(text)] + [(pack, "gode_pack_op")])


def _wrap(head, items, indent, tail):
    """head + the comma-separated items + tail, wrapped at ~110 columns."""
    row, rows = head, []
    for item in items:
        if len(row) + len(item) + 2 > 112:
            rows.append(row.rstrip())
            row = indent
        row += item + ", "
    return rows + [row.rstrip(", ") + tail]


def generate():
    text = open(HEADER).read()
    structs = parse_structs(text)
    kinds = parse_kinds(text)
    names = {n for n, _ in structs}
    lines = ["import ctypes as C", "", "i32, i64, f32, ptr = C.c_int32, C.c_int64, C.c_float, C.c_void_p", ""]
    for name, fields in structs:
        lines.append(f"class {name}(C.Structure):")
        lines += _wrap("    _fields_ = [", [f'("{f}", {t})' for f, t in fields], " " * 16, "]") + [""]
    lines.append("KINDS = {0: gode_conv_geom, -1: gode_adam_noise_tensor, " + ", ".join(f"{v}: {st}" for v, st in kinds) + "}")
    lines += ["", "",
              "def load(path=\"gan-ode_amd/lib/libgode.so\"):",
              "    lib = C.CDLL(path)",
              "    lib.gode_sizeof.argtypes = [C.c_int]",
              "    for kind, st in KINDS.items():            # the mirror must match the compiled ABI, field for field",
              "        assert lib.gode_sizeof(kind) == C.sizeof(st), (kind, st.__name__)"]
    lines += _wrap("    for fn in (", [f'"{fn}"' for _, _, _, fn in parse_ops(text)], " " * 15, "):")
    lines += ["        getattr(lib, fn).argtypes = [ptr, ptr]          # (const op struct*, hipStream_t)",
              "        getattr(lib, fn).restype = C.c_int              # 0 ok, <0 GODE_E_*, >0 hipError_t",
              "    return lib"]
    missing = [st for _, st in kinds if st not in names]
    assert not missing, missing
    return "\n".join(lines) + "\n"


def main():
    stub = generate()
    if "--write" in sys.argv:
        doc = open(DOC).read()
        i, j = doc.index(BEGIN), doc.index(END)
        doc = doc[:i] + BEGIN + "\n```python\n" + stub + "```\n" + doc[j:]
        open(DOC, "w").write(doc)
        print("rewrote", DOC)
    else:
        sys.stdout.write(stub)


if __name__ == "__main__":
    main()
