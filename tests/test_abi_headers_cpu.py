"""Holds the ctypes binding (gsrast/_abi.py) to the two public headers, without a GPU: tests/abi_header.py parses include/gsrast.h and
include/gsdecode.h, and the table of entry points, the Structure mirrors and every constant that Python restates have to agree with what it reads."""
import ctypes as C

import pytest

import abi_header as H

SRC = {h: H.source(h) for h in H.HEADERS}
CONSTS = {k: v for h in H.HEADERS for k, v in H.constants(SRC[h]).items()}
PROTOS = {h: H.functions(SRC[h]) for h in H.HEADERS}
FIELDS = {h: H.structs(SRC[h]) for h in H.HEADERS}
ALL_PROTOS = {k: v for h in H.HEADERS for k, v in PROTOS[h].items()}
ALL_FIELDS = {k: v for h in H.HEADERS for k, v in FIELDS[h].items()}
RESTYPES = {("size_t", 0): C.c_size_t, ("int", 0): C.c_int, ("int32_t", 0): C.c_int32, ("uint32_t", 0): C.c_uint32, ("char", 1): C.c_char_p}


def _scalar(ct):
    """(bytes, is a float, is signed) of a ctypes number; None for anything else (pointers, c_void_p, c_char_p, structs, arrays)."""
    code = getattr(ct, "_type_", None)
    if not (isinstance(ct, type) and issubclass(ct, C._SimpleCData) and isinstance(code, str) and code in "bBhHiIlLqQfd"):
        return None
    return C.sizeof(ct), code in "fd", code in "fd" or code.islower()


def _pointer_ok(bound, base, structs):
    """A pointer parameter to `base` accepts void*, POINTER(scalar of that type) and POINTER(the mirror of that struct), nothing else."""
    if bound is C.c_void_p:
        return True
    if not (isinstance(bound, type) and issubclass(bound, C._Pointer)):
        return False
    if base in structs:
        return bound._type_ is structs[base]
    return base in H.SCALARS and _scalar(bound._type_) == _scalar(H.SCALARS[base])


def check_function(name, proto, row, structs):
    """None, or what is wrong with the table row (restype, argtypes) of the prototype (return type, parameter types)."""
    (rbase, rdepth), params = proto
    restype, argtypes = row
    want = RESTYPES.get((rbase, rdepth))
    if want is None:
        return f"{name}: a return type the binding has no rule for: {rbase}{'*' * rdepth}"
    if restype is not want and (want is C.c_char_p or _scalar(restype) != _scalar(want)):
        return f"{name}: returns {rbase}{'*' * rdepth} but is bound as {restype}"
    if argtypes is None or len(argtypes) != len(params):
        return f"{name}: {len(params)} parameters but {None if argtypes is None else len(argtypes)} argtypes"
    for i, ((base, depth), bound) in enumerate(zip(params, argtypes)):
        if depth == 0:
            ok = base in H.SCALARS and _scalar(bound) == _scalar(H.SCALARS[base])
        else:
            ok = depth == 1 and _pointer_ok(bound, base, structs)
        if not ok:
            return f"{name}: parameter {i} is {base}{'*' * depth} but is bound as {bound}"
    return None


def check_struct(name, mirror, built, fields, structs):
    """None, or how the mirror differs from the struct ctypes lays out from the header's fields: names in order, offsets, sizes, sizeof, and the
    kind of every field (a number or an array as in the header, a nested struct as its own mirror, a pointer as some pointer)."""
    layout = lambda t: [(n, getattr(t, n).offset, getattr(t, n).size) for n, _ in t._fields_]
    if layout(mirror) != layout(built) or C.sizeof(mirror) != C.sizeof(built):
        return f"{name}: header {layout(built)} sizeof {C.sizeof(built)}, mirror {layout(mirror)} sizeof {C.sizeof(mirror)}"
    for (field, base, depth, length), (_, mt), (_, bt) in zip(fields, mirror._fields_, built._fields_):
        et = mt._type_ if length is not None and issubclass(mt, C.Array) else mt
        if depth:
            ok = et is C.c_void_p or issubclass(et, C._Pointer)
        elif base in H.SCALARS:
            ok = _scalar(et) == _scalar(H.SCALARS[base])
        else:
            ok = et is structs[base]
        if not ok or (length is not None and not issubclass(mt, C.Array)):
            return f"{name}.{field}: header {base}{'*' * depth}{'' if length is None else '[' + length + ']'} but the mirror has {mt}"
    return None


def test_the_parser_reads_everything_and_the_table_covers_it():
    from gsrast import _abi, decode
    import gsrast
    for h in H.HEADERS:
        assert set(PROTOS[h]) == H.loose_functions(SRC[h]), h
        assert len(FIELDS[h]) == H.count_typedef_structs(SRC[h]), h
    names = [row[0] for row in _abi.FUNCTIONS]
    assert len(names) == len(set(names)), "a function has two rows"
    assert set(names) == set(ALL_PROTOS), (set(names) ^ set(ALL_PROTOS))
    assert set(_abi.STRUCTS) == set(ALL_FIELDS), (set(_abi.STRUCTS) ^ set(ALL_FIELDS))
    assert all(s.__name__ == k for k, s in _abi.STRUCTS.items())
    assert sorted(gsrast.EXPORTS) == sorted(PROTOS["gsrast.h"])
    decl = sorted(PROTOS["gsdecode.h"])
    assert sorted(decode.EXPORTS) == decl and len(decl) == 13


def test_every_row_matches_its_prototype():
    from gsrast import _abi
    rows = {name: (restype, argtypes) for name, restype, argtypes in _abi.FUNCTIONS}
    wrong = [w for w in (check_function(n, ALL_PROTOS[n], rows[n], _abi.STRUCTS) for n in sorted(ALL_PROTOS)) if w]
    assert not wrong, "\n".join(wrong)


def test_every_mirror_matches_its_struct():
    from gsrast import _abi
    built = H.build_structs(ALL_FIELDS, CONSTS)
    wrong = [w for w in (check_struct(n, _abi.STRUCTS[n], built[n], ALL_FIELDS[n], _abi.STRUCTS) for n in ALL_FIELDS) if w]
    assert not wrong, "\n".join(wrong)


def test_the_checks_refuse_what_they_are_there_for():
    """The two checkers on hand-made rows and mirrors that are wrong in one way each, so that a checker that accepts everything is seen here."""
    from gsrast import _abi
    S, vp, i32, sz, P = _abi.STRUCTS, C.c_void_p, C.c_int32, C.c_size_t, C.POINTER
    proto = ALL_PROTOS["gsr_forward_stage1"]              # (cfg*, inputs*, void*, size_t, int32_t*, uint32_t*, void*) -> int
    cfg, inp = P(S["gsr_cfg"]), P(S["gsr_inputs"])
    good = [cfg, inp, vp, sz, vp, P(C.c_uint32), vp]
    assert check_function("f", proto, (C.c_int, good), S) is None
    assert check_function("f", proto, (C.c_int, [vp, vp, vp, sz, P(i32), vp, vp]), S) is None
    for restype, argtypes in ((C.c_int, [inp, cfg] + good[2:]),                       # two struct pointers exchanged
                              (C.c_int, [cfg, inp, sz, vp] + good[4:]),               # a pointer and a size exchanged
                              (C.c_int, good[:3] + [i32] + good[4:]),                 # size_t as int32
                              (C.c_int, good[:3] + [C.c_int64] + good[4:]),           # size_t as a signed 64-bit number
                              (C.c_int, good[:5] + [P(C.c_uint64), vp]),              # uint32_t* as uint64_t*
                              (C.c_int, good[:5] + [P(C.c_float), vp]),               # uint32_t* as float*
                              (C.c_int, good[:-1]), (C.c_int, None),                  # an argument short, no argtypes
                              (sz, good), (C.c_char_p, good)):                        # the wrong return type
        assert check_function("f", proto, (restype, argtypes), S) is not None, (restype, argtypes)
    assert check_function("f", ALL_PROTOS["gsr_geom_bytes"], (C.c_int, [i32, i32]), S) is not None          # size_t read as int
    assert check_function("f", ALL_PROTOS["gsr_adam_step"], (C.c_int, [C.c_int64, vp, vp, vp, vp] + [C.c_float] * 5 + [vp, vp]), S) is not None   # double as float
    built = H.build_structs(ALL_FIELDS, CONSTS)
    fields = list(S["gsr_mv_cfg"]._fields_)
    swapped = fields[:5] + [fields[6], fields[5]] + fields[7:]                        # Hg (int32) and fx (float) exchanged: same layout, other names and kinds
    arrays = fields[:14] + [fields[15], fields[14]] + fields[16:]                     # v2n and n2v exchanged: names only
    for wrong in (swapped, arrays, fields[:-1], fields[:14] + [("v2n", C.c_float * 11)] + fields[15:]):
        m = type("gsr_mv_cfg", (C.Structure,), {"_fields_": wrong})
        assert check_struct("gsr_mv_cfg", m, built["gsr_mv_cfg"], ALL_FIELDS["gsr_mv_cfg"], S) is not None
    kinds = [(n, C.c_int32 if n == "fx" else t) for n, t in fields]                   # a float read as an int32: the layout alone does not see it
    assert check_struct("gsr_mv_cfg", type("gsr_mv_cfg", (C.Structure,), {"_fields_": kinds}), built["gsr_mv_cfg"], ALL_FIELDS["gsr_mv_cfg"], S) is not None


def test_restated_constants_equal_the_headers():
    import gsrast
    from gsrast import _rows, init, mesh, views
    assert gsrast.ABI_VERSION == CONSTS["GSR_ABI_VERSION"]
    assert (gsrast.EWA, gsrast.SURFEL, gsrast.PLANE) == (CONSTS["GSR_EWA"], CONSTS["GSR_SURFEL"], CONSTS["GSR_PLANE"])
    assert gsrast.TsdfSparse.MAX_CHUNKS == CONSTS["GSR_TSDF_MAX_CHUNKS"]
    assert _rows.WEED_CHUNK == CONSTS["GSR_OCTREE_WEED_CHUNK"]
    assert views.MAX_IMAGES == CONSTS["GSR_VIEWS_MAX_IMAGES"]
    for mod, prefix, message in ((views, "GSR_VIEWS_ERR_", views.status_message), (init, "GSR_INIT_ERR_", lambda s: init.status_message("x", s))):
        bits = {k[len(prefix):]: v for k, v in CONSTS.items() if k.startswith(prefix)}
        assert bits and all(getattr(mod, "ERR_" + k) == v for k, v in bits.items()), (prefix, bits)
        assert all("unknown bits" not in message(v) for v in bits.values())           # every bit of the header is decoded
        assert "unknown bits" in message(max(bits.values()) << 1)                     # and no bit beyond them
    for prefix, short in (("GSR_MESH_DROP_", "DROP_"), ("GSR_MESH_ERR_", "ERR_")):
        bits = {k[len(prefix):]: v for k, v in CONSTS.items() if k.startswith(prefix)}
        assert bits and all(getattr(mesh, short + k) == v for k, v in bits.items()), (prefix, bits)
    from gsrast import densify, tsdf
    assert (densify.SIZE_PRUNE, densify.CLONE_CAP, densify.SPLIT_CAP, densify.ABS_CAP) == \
        (CONSTS["GSR_DEN_SIZE_PRUNE"], CONSTS["GSR_DEN_CLONE_CAP"], CONSTS["GSR_DEN_SPLIT_CAP"], CONSTS["GSR_DEN_ABS_CAP"])
    assert tsdf.ScalableTSDFVolume.TSDF_NO_SYNC == CONSTS["GSR_TSDF_NO_SYNC"]
    assert len(gsrast.PROF_LABELS) == CONSTS["GSR_PROF_LABELS"]
    stages = {k[len("GSR_PROF_"):].lower(): v for k, v in CONSTS.items() if k.startswith("GSR_PROF_") and k != "GSR_PROF_LABELS"}
    assert stages and all(gsrast.PROF_LABELS[v] == k for k, v in stages.items())


def test_the_loaded_library_has_every_signature():
    import gsrast
    from gsrast import _abi
    L = gsrast.lib()
    for name, restype, argtypes in _abi.FUNCTIONS:
        f = getattr(L, name)
        assert f.argtypes is not None and list(f.argtypes) == list(argtypes) and f.restype is restype, name

    class Empty:
        pass
    with pytest.raises(RuntimeError, match=r"does not export gsr_geom_bytes.*rebuild"):
        _abi.bind(Empty(), "libgsrast_hip.so")
