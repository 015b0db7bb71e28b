"""How the refused calls of tests/golden/refusals.json are made (tests/test_refusals.py replays them, tests/golden/make_refusals.py
recorded them): every public function of the fifteen derived Python modules with the library out of reach, and every public C entry
of the fifteen derived units through ctypes, each with one named fault or two in its arguments.  An entry is "py:<module>.<function>"
or "c:<symbol>"; a case is an entry and the names of its faults; its message is the exception's type and text, or the C library's
last-error text.  Only calls that are refused before any HIP call are in the table, so it reads the same with and without a GPU."""
import ctypes
import importlib
import inspect

import numpy as np

MODULES = ("wide", "where", "filter", "filter_where", "wide_filter", "wide_where", "wide_filter_where", "segments", "segments_filter",
           "segments_where", "segments_filter_where", "segments_wide", "segments_wide_filter", "segments_wide_where",
           "segments_wide_filter_where")
N = 10   # elements of every array of a Python case


class LibraryTouched(Exception):
    """the call reached _lib.lib(): it was not refused by the Python layer"""


# ------------------------------------------------------------------ Python entries
def py_entries():
    """"py:<module>.<function>" of every public function of the fifteen modules that is defined there"""
    out = []
    for m in MODULES:
        mod = importlib.import_module("libflagstats_amd." + m)
        for name, f in sorted(vars(mod).items()):
            if inspect.isfunction(f) and f.__module__ == mod.__name__ and not name.startswith("_"):
                out.append("py:%s.%s" % (m, name))
    return out


def _kind(name, params):
    return "torch" if "t" in params else "ptr" if "ptr" in params else "numpy" if "values" in params else "helper"


def py_base(entry):
    """the function and keyword arguments that the Python layer accepts (the torch entries go on to refuse their CPU tensors)"""
    import torch
    m, name = entry[3:].split(".")
    f = getattr(importlib.import_module("libflagstats_amd." + m), name)
    params = inspect.signature(f).parameters
    kind = _kind(name, params)
    wide = "wide" in m
    kw = {}
    if kind == "helper":
        kw = {"lengths": [3, 7], "offsets": [0, 4, N], "n": N, "counters": np.zeros((2, 32), dtype=np.uint64),
              "selected": np.zeros(2, dtype=np.uint64), "high": np.array([0, 1 << 16], dtype=np.uint64), }
        return f, {k: v for k, v in kw.items() if k in params}, kind
    if kind == "torch":
        kw["t"] = torch.zeros(N, dtype=torch.int32 if wide else torch.int16)
        if "offsets" in params:
            kw["offsets"] = torch.tensor([0, 4, N], dtype=torch.int64)
        if "where" in params:
            kw["where"] = torch.zeros(N, dtype=torch.bool)
    elif kind == "numpy":
        kw["values"] = np.zeros(N, dtype=np.int32 if wide else np.uint16)
        if "offsets" in params:
            kw["offsets"] = [0, 4, N]
        if "where" in params:
            kw["where"] = np.zeros(N, dtype=bool)
    else:
        kw.update(ptr=0x1000, n=N)
        for k, v in (("elem_bytes", 4), ("offsets", [0, 4, N]), ("sel_ptr", 0x2000), ("sel_bits", 8)):
            if k in params:
                kw[k] = v
    return f, kw, kind


def _py_faults(kind, params):
    """(name, keyword overrides) of every fault the function's parameters allow, in a fixed order"""
    import torch
    T = kind == "torch"
    z = (lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, dt))) if T else (lambda shape, dt: np.zeros(shape, dtype=dt))
    F = []
    if "values" in params:
        F += [("values_type", dict(values=[1, 2, 3])), ("values_dtype", dict(values=np.zeros(N, dtype=np.float32))),
              ("values_int8", dict(values=np.zeros(N, dtype=np.int8))), ("values_byteorder", dict(values=np.zeros(N, dtype=">i4"))),
              ("values_ndim", dict(values=np.zeros((2, 5), dtype=np.uint16)))]
    if "t" in params:
        F += [("t_type", dict(t=np.zeros(N, dtype=np.int16))), ("t_dtype", dict(t=torch.zeros(N, dtype=torch.float32))),
              ("t_uint8", dict(t=torch.zeros(N, dtype=torch.uint8))), ("t_ndim", dict(t=torch.zeros((2, 5), dtype=torch.int16)))]
    if "where" in params:
        F += [("where_type", dict(where=[True] * N)), ("where_ndim", dict(where=z((2, 5), "bool"))),
              ("where_dtype", dict(where=z(N, "uint8"))), ("where_size", dict(where=z(N - 1, "bool"))),
              ("packed_dtype", dict(packed=True)), ("packed_short", dict(packed=True, where=z(1, "uint8"), bit_offset=7)),
              ("bit_offset_type", dict(bit_offset=1.5)), ("bit_offset_negative", dict(bit_offset=-1)),
              ("bit_offset_unpacked", dict(bit_offset=3))]
    if "mapq" in params:
        F += [("mapq_type", dict(mapq=[0] * N, min_mapq=1)), ("mapq_dtype", dict(mapq=z(N, "int32"), min_mapq=1)),
              ("mapq_ndim", dict(mapq=z((2, 5), "uint8"), min_mapq=1)), ("mapq_size", dict(mapq=z(N - 1, "uint8"), min_mapq=1))]
    if "require" in params:
        F += [("require_type", dict(require=1.5)), ("require_range", dict(require=0x10000)), ("exclude_type", dict(exclude="1")),
              ("exclude_range", dict(exclude=-1)), ("min_mapq_type", dict(min_mapq=2.5)), ("min_mapq_range", dict(min_mapq=256)),
              ("min_mapq_needs_mapq", dict(min_mapq=30))]
    if "offsets" in params and T:
        F += [("offsets_type", dict(offsets=np.array([0, N]))), ("offsets_dtype", dict(offsets=torch.tensor([0, N], dtype=torch.int32))),
              ("offsets_empty", dict(offsets=torch.zeros(0, dtype=torch.int64)))]
    elif "offsets" in params:
        F += [("offsets_ndim", dict(offsets=np.array([[0, 5], [5, N]]))), ("offsets_empty", dict(offsets=np.array([], dtype=np.uint64))),
              ("offsets_dtype", dict(offsets=np.array([0.0, 5.0, 10.0]))), ("offsets_negative", dict(offsets=np.array([-1, 5, N]))),
              ("offsets_decreasing", dict(offsets=[0, 5, 3, N])), ("offsets_exceed", dict(offsets=[0, 5, N + 1]))]
    if kind == "ptr":
        F += [("ptr_type", dict(ptr=1.5)), ("ptr_big", dict(ptr=1 << 64)), ("n_type", dict(n=2.5)), ("n_negative", dict(n=-1))]
        if "elem_bytes" in params:
            F += [("elem_bytes_2", dict(elem_bytes=2)), ("elem_bytes_3", dict(elem_bytes=3))]
        if "sel_bits" in params:
            F += [("sel_bits_4", dict(sel_bits=4)), ("sel_bits_bool", dict(sel_bits=True)), ("sel_ptr_type", dict(sel_ptr="x")),
                  ("sel_offset_negative", dict(sel_offset=-1))]
        if "mapq_ptr" in params:
            F += [("mapq_ptr_type", dict(mapq_ptr=1.0))]
    if T:
        F += [("out_type", dict(out=np.zeros(32, dtype=np.int64))), ("out_shape", dict(out=torch.zeros(5, dtype=torch.int64)))]
        for k in ("selected", "high"):
            if k in params:
                F += [(k + "_shape", dict(**{k: torch.zeros(7, dtype=torch.int64)})), (k + "_dtype", dict(**{k: torch.zeros(1, dtype=torch.int32)}))]
        F += [("cpu_tensor", {})]
    if kind == "helper":
        F += [("lengths_ndim", dict(lengths=[[1, 2]])), ("lengths_negative", dict(lengths=[1, -2])), ("lengths_float", dict(lengths=[1.5])),
              ("counters_shape", dict(counters=np.zeros((2, 31)))), ("selected_size", dict(selected=np.zeros(3)))]
    return [(name, o) for name, o in F if set(o) <= set(params)]


# ------------------------------------------------------------------ C entries
def c_units():
    """(x64, sync, device) symbols and the axes (wide, segments, filter, where) of the fifteen units"""
    out = []
    for wide in (False, True):
        for seg in (False, True):
            for filt in (False, True):
                for where in (False, True):
                    if not (wide or seg or filt or where):
                        continue   # K1
                    kind = "wide" if wide else "u16"
                    sfx = ("_segments" if seg else "") + ("_filter" if filt else "") + ("_where" if where else "")
                    dev = "FLAGSTATS_hip_device_%s%s" % (kind, sfx)
                    out.append((("FLAGSTATS_hip_%s_x64%s" % (kind, sfx), dev + "_sync", dev), (wide, seg, filt, where)))
    return out


def c_entries():
    return ["c:" + name for names, _ in c_units() for name in names]


_KEEP = []   # the buffers of the C cases


def _c_buffers():
    if not _KEEP:
        _KEEP.extend([np.zeros(104, dtype=np.int64), np.array([0, 40, 100], dtype=np.uint64), np.zeros(100, dtype=np.uint8),
                      np.zeros(100, dtype=np.uint8), np.full((2, 32), 7, dtype=np.uint64), np.full(2, 7, dtype=np.uint64),
                      np.full(2, 7, dtype=np.uint64)])
    return _KEEP


def c_call(entry, faults):
    """the C entry under the named faults: its return value and the last-error text"""
    from libflagstats_amd import _lib
    lib = _lib.lib()
    name = entry[2:]
    (names, (wide, seg, filt, where)), = [u for u in c_units() if name in u[0]]
    a, o, q, s, out, sel, high = _c_buffers()
    v = dict(array=a.ctypes.data, n=100, eb=8, offsets=o.ctypes.data, nseg=2, require=1, exclude=4, mapq=q.ctypes.data, min_mapq=30,
             sel=s.ctypes.data, sel_offset=0, sel_bits=8, out=out.ctypes.data, selected=sel.ctypes.data, high=high.ctypes.data, flags=1)
    table = dict(C_FAULTS)
    for fname in faults:
        v.update(table[fname](v, wide))
    args = [v["array"], v["n"]] + ([v["eb"]] if wide else []) + ([v["offsets"], v["nseg"]] if seg else [])
    args += ([v["require"], v["exclude"], v["mapq"], v["min_mapq"]] if filt else []) + ([v["sel"], v["sel_offset"], v["sel_bits"]] if where else [])
    args += [v["out"]] + ([v["selected"]] if filt or where else []) + ([v["high"]] if wide else []) + [v["flags"]]
    if name == names[2]:
        args.append(None)   # the stream
    rc = getattr(lib, name)(*args)
    text = lib.FLAGSTATS_hip_last_error().decode() if rc else ""
    assert (out == 7).all() and (sel == 7).all() and (high == 7).all(), (entry, faults)
    return rc, text


# name -> (values, wide) -> overrides; in the order the units ask (the base segmented unit's three entries differ, and say so)
C_FAULTS = (
    ("elem_bytes_2", lambda v, w: dict(eb=2)), ("elem_bytes_3", lambda v, w: dict(eb=3)),
    ("require", lambda v, w: dict(require=0x10000)), ("exclude", lambda v, w: dict(exclude=0x10000)),
    ("min_mapq", lambda v, w: dict(min_mapq=256)), ("sel_bits", lambda v, w: dict(sel_bits=4)), ("flags", lambda v, w: dict(flags=4)),
    ("null_offsets", lambda v, w: dict(offsets=None)), ("null_out", lambda v, w: dict(out=None)),
    ("nseg_huge", lambda v, w: dict(nseg=1 << 60)), ("null_array", lambda v, w: dict(array=None)),
    ("null_mapq", lambda v, w: dict(mapq=None)), ("null_sel", lambda v, w: dict(sel=None)),
    ("misaligned", lambda v, w: dict(array=v["array"] + (4 if w else 1))), ("misaligned_4", lambda v, w: dict(array=v["array"] + 2, eb=4)),
    ("n_size", lambda v, w: dict(n=(1 << 64) // (8 if w else 2))), ("sel_range", lambda v, w: dict(sel_offset=(1 << 64) - 120)),
)
C_FAULT_KEYS = {"elem_bytes_2": {"eb"}, "elem_bytes_3": {"eb"}, "require": {"require"}, "exclude": {"exclude"}, "min_mapq": {"min_mapq"},
                "sel_bits": {"sel_bits"}, "flags": {"flags"}, "null_offsets": {"offsets"}, "null_out": {"out"}, "nseg_huge": {"nseg"},
                "null_array": {"array"}, "null_mapq": {"mapq"}, "null_sel": {"sel"}, "misaligned": {"array"},
                "misaligned_4": {"array", "eb"}, "n_size": {"n"}, "sel_range": {"sel_offset"}}


def c_faults(entry):
    """the faults the entry's *_args refuses (what it would only refuse after a HIP call is left out)"""
    name = entry[2:]
    (names, (wide, seg, filt, where)), = [u for u in c_units() if name in u[0]]
    base = seg and not (wide or filt or where)
    keep = {"flags", "null_array"}
    keep |= {"elem_bytes_2", "elem_bytes_3", "misaligned_4"} if wide else set()
    keep |= {"require", "exclude", "min_mapq", "null_mapq"} if filt else set()
    keep |= {"sel_bits", "null_sel", "sel_range"} if where else set()
    keep |= {"null_offsets", "null_out", "nseg_huge"} if seg else {"null_out"}
    if not base:
        keep |= {"misaligned", "n_size"}
    elif name != names[0]:
        keep |= {"misaligned"}
    return [n for n, _ in C_FAULTS if n in keep]


# ------------------------------------------------------------------ both
def load_golden(path):
    """(entry, [fault names], message) of every case of refusals.json: the entries that answer alike share a table; a pair written
    "a>b" is both faults giving a's message, [a, b, i] both giving message i"""
    import json
    with open(path) as f:
        doc = json.load(f)
    msg = doc["messages"]
    cases = []
    for table in doc["tables"]:
        for entry in table["entries"]:
            cases += [(entry, [name], msg[i]) for name, i in table["single"].items()]
            for p in table["pairs"]:
                if isinstance(p, str):
                    a, b = p.split(">")
                    cases.append((entry, [a, b], msg[table["single"][a]]))
                else:
                    cases.append((entry, p[:2], msg[p[2]]))
    return cases


def faults_of(entry):
    """(name, the set of arguments it changes) of the entry's faults"""
    if entry.startswith("c:"):
        return [(n, C_FAULT_KEYS[n]) for n in c_faults(entry)]
    f, kw, kind = py_base(entry)
    return [(n, set(o) or {"-"}) for n, o in _py_faults(kind, inspect.signature(f).parameters)]


def message(entry, faults):
    """what the entry answers under the named faults: "<exception type>: <text>" or the C last-error text; None where it does not
    refuse (LibraryTouched is raised where the Python layer went on to the library)"""
    if entry.startswith("c:"):
        rc, text = c_call(entry, faults)
        return text if rc else None
    f, kw, kind = py_base(entry)
    table = dict(_py_faults(kind, inspect.signature(f).parameters))
    for name in faults:
        kw.update(table[name])
    try:
        f(**kw)
    except LibraryTouched:
        raise
    except Exception as e:   # noqa: BLE001  (the type is part of what is recorded)
        return "%s: %s" % (type(e).__name__, e)
    return None
