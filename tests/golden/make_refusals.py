"""Records tests/golden/refusals.json: run at the commit whose refusals are to be pinned, with the library built.

For every entry of tests/refusal_cases.py it keeps the faults that are refused before any HIP call (Python: a ValueError raised
before _lib.lib() is reached), finds the order in which the entry asks for them from the calls with two faults, and writes one
case per single fault and one per pair of neighbours in that order whose faults change different arguments and give different
messages -- so the file pins every text and the order of the checks.  A fault that is not refused is not in the file."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import refusal_cases as rc  # noqa: E402
from libflagstats_amd import _lib  # noqa: E402


def answer(entry, faults, real_lib):
    """the message of a refusal that comes before the library (Python) or before any HIP call (C), else None"""
    if entry.startswith("c:"):
        _lib.lib = real_lib
        text = rc.message(entry, faults)
        # past its argument checks an entry asks the runtime about its pointers; that failure speaks of something else
        about = ("elem_bytes", "require ", "exclude ", "min_mapq ", "sel_bits ", "flags:", "NULL ", "nseg ", "array must", "n * ", "sel_offset ")
        return text if text is not None and text.replace("libflagstats_hip: ", "", 1).startswith(about) else None
    def boom():
        raise rc.LibraryTouched()
    _lib.lib = boom
    try:
        text = rc.message(entry, faults)
    except rc.LibraryTouched:
        return None
    finally:
        _lib.lib = real_lib
    return text if text is not None and text.startswith("ValueError: ") else None


def cases_of(entry, real_lib):
    faults = rc.faults_of(entry)
    single = {}
    for name, _ in faults:
        text = answer(entry, [name], real_lib)
        if text is not None:
            single[name] = text
    names = [n for n, _ in faults if n in single]
    keys = dict(faults)
    beaten = {n: 0 for n in names}   # how many faults are reported in front of n
    pair = {}
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            if keys[a] & keys[b] or single[a] == single[b]:
                continue
            text = answer(entry, [a, b], real_lib)
            pair[a, b] = text
            if text == single[a]:
                beaten[b] += 1
            elif text == single[b]:
                beaten[a] += 1
    order = sorted(names, key=lambda n: (beaten[n], names.index(n)))
    out = [(entry, [n], single[n]) for n in order]
    for i, a in enumerate(order):
        for b in order[i + 1:]:
            text = pair.get((a, b), pair.get((b, a)))
            if text is not None:
                out.append((entry, [a, b], text))
                break
    return out


def main():
    real_lib = _lib.lib
    real_lib()
    cases = []
    for entry in rc.py_entries() + rc.c_entries():
        cases += cases_of(entry, real_lib)
    # The file (rc.load_golden reads it back): the distinct messages; then one table per set of entries that answer alike --
    # "single": fault -> message, "pairs": "a>b" where both faults give a's message, [a, b, message] where they give a third.
    messages = sorted({text for _, _, text in cases})
    index = {text: i for i, text in enumerate(messages)}
    tables = {}
    for entry in dict.fromkeys(e for e, _, _ in cases):
        mine = [(f, index[text]) for e, f, text in cases if e == entry]
        single = {f[0]: i for f, i in mine if len(f) == 1}
        pairs = ["%s>%s" % ((a, b) if i == single[a] else (b, a)) if i in (single[a], single[b]) else [a, b, i]
                 for (a, b), i in (x for x in mine if len(x[0]) == 2)]
        tables.setdefault(json.dumps({"single": single, "pairs": pairs}, separators=(",", ":")), []).append(entry)
    with open(os.path.join(HERE, "refusals.json"), "w") as f:
        f.write('{"messages":[\n' + ",\n".join(json.dumps(m) for m in messages) + '\n],\n"tables":[\n')
        f.write(",\n".join('{"entries":%s,%s' % (json.dumps(e, separators=(",", ":")), t[1:]) for t, e in tables.items()))
        f.write("\n]}\n")
    print(len(cases), "cases,", len(messages), "messages,", len({e for e, _, _ in cases}), "entries,", len(tables), "tables")


if __name__ == "__main__":
    main()
