"""A small parser of include/gsrast.h and include/gsdecode.h for tests/test_abi_headers_cpu.py: prototypes, `typedef struct` bodies, #define and
enum constants, and each struct rebuilt with ctypes from what was parsed.  It reads the subset of C the two headers use and refuses the rest:
a declaration it cannot read raises, and the test compares what it found with a loose regex over the same text, so nothing is skipped silently."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("gsrast.h", "gsdecode.h")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8,
           "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}


def source(header):
    """The header's text without its comments."""
    with open(os.path.join(ROOT, "include", header)) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def loose_functions(src):
    """Every gsr_ / gsd_ name that is followed by an opening parenthesis: what tests/test_abi_cpu.py has always taken for the declared symbols."""
    return set(re.findall(r"\b(gs[rd]_\w+)\s*\(", src))


def count_typedef_structs(src):
    return len(re.findall(r"^\s*typedef\s+struct\b", src, flags=re.M))


def _type(text):
    """'const gsr_cfg*' -> ('gsr_cfg', 1): the base type's name and the pointer depth; const is dropped."""
    words = re.sub(r"\bconst\b", " ", text).replace("*", " * ").split()
    base = [w for w in words if w != "*"]
    if len(base) != 1 or not re.fullmatch(r"\w+", base[0]):
        raise ValueError(f"cannot read the type '{text.strip()}'")
    return base[0], words.count("*")


def constants(src):
    """{name: int} of the #defines with an integer value and of every enumerator."""
    out = {}
    for name, value in re.findall(r"^\s*#define\s+(\w+)\s+(\d+)[uU]?\s*$", src, flags=re.M):
        out[name] = int(value)
    for body in re.findall(r"\benum\b\s*\w*\s*\{(.*?)\}", src, flags=re.S):
        nxt = 0
        for item in filter(None, (x.strip() for x in body.split(","))):
            m = re.fullmatch(r"(\w+)(?:\s*=\s*(\d+))?", item)
            if not m:
                raise ValueError(f"cannot read the enumerator '{item}'")
            nxt = int(m.group(2)) if m.group(2) is not None else nxt
            out[m.group(1)] = nxt
            nxt += 1
    return out


def structs(src):
    """{struct name: [(field, base type, pointer depth, array length or None)]} in the header's order; array lengths stay as written."""
    out = {}
    for tag, body, name in re.findall(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        if tag != name:
            raise ValueError(f"struct {tag} is typedef'd as {name}")
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"((?:const\s+)?\w+)\b(.*)", decl, flags=re.S)
            if not m:
                raise ValueError(f"{name}: cannot read '{decl}'")
            base, base_depth = _type(m.group(1))
            for d in m.group(2).split(","):
                dm = re.fullmatch(r"\s*(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", d)
                if not dm:
                    raise ValueError(f"{name}: cannot read the declarator '{d}' of '{decl}'")
                fields.append((dm.group(2), base, base_depth + len(dm.group(1)), dm.group(3)))
        out[name] = fields
    return out


def functions(src):
    """{name: (return type, [parameter type])}, a type being (base, pointer depth), from the text left once the preprocessor lines, the struct and enum
    bodies and the extern "C" braces are taken out: every remaining statement has to read as a prototype."""
    text = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    text = re.sub(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = re.sub(r"\benum\b\s*\w*\s*\{.*?\}\s*;", "", text, flags=re.S)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    out = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        if stmt == "}":                                   # closes extern "C"
            continue
        m = re.fullmatch(r"(.*?)\b(gs[rd]_\w+)\s*\((.*)\)", stmt, flags=re.S)
        if not m or "(" in m.group(3):
            raise ValueError(f"cannot read the statement '{stmt}'")
        params = []
        if m.group(3).strip() != "void":
            for p in m.group(3).split(","):
                pm = re.fullmatch(r"(.*?)(\w+)\s*", p, flags=re.S)            # the type, then the parameter's name
                if not pm:
                    raise ValueError(f"{m.group(2)}: cannot read the parameter '{p}'")
                params.append(_type(pm.group(1)))
        if m.group(2) in out:
            raise ValueError(f"{m.group(2)} is declared twice")
        out[m.group(2)] = (_type(m.group(1)), params)
    return out


def build_structs(parsed, consts):
    """{name: ctypes.Structure subclass} laid out by ctypes from the parsed fields alone: a pointer of any kind is a void*, an array length is a number or
    a #define, a nested struct is the one built before it."""
    built = {}
    for name, fields in parsed.items():
        ct_fields = []
        for field, base, depth, length in fields:
            if depth:
                ct = C.c_void_p
            elif base in SCALARS:
                ct = SCALARS[base]
            else:
                ct = built[base]                          # KeyError: an unknown type, or a struct used before its definition
            if length is not None:
                ct = ct * (int(length) if length.isdigit() else consts[length])
            ct_fields.append((field, ct))
        built[name] = type(name, (C.Structure,), {"_fields_": ct_fields})
    return built
