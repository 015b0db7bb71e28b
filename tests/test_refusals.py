"""The refusals of the derived entries are what they were: tests/golden/refusals.json (recorded by tests/golden/make_refusals.py
before the argument rules were gathered into one place) holds, for every public function of the fifteen derived Python modules and
every public C entry of the fifteen derived units, the exact message under each single fault of its arguments and under pairs of
faults that pin the order of its checks.  Every case is refused before any HIP call -- the Python ones before the library is even
loaded -- so the file reads the same with and without a GPU.  No case is skipped: the number replayed is the number recorded."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refusal_cases as rc  # noqa: E402

GOLDEN = rc.load_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusals.json"))   # (entry, faults, message)
NO_REFUSALS = {"py:wide.high_bits_message", "py:segments_wide.strict_message"}   # they format a message and refuse nothing


def test_the_table_covers_every_entry():
    recorded = {entry for entry, _, _ in GOLDEN}
    assert recorded == (set(rc.py_entries()) | set(rc.c_entries())) - NO_REFUSALS
    assert len(rc.c_entries()) == 45 and len(rc.py_entries()) == 64
    # every entry has its single faults and, where two of them change different arguments and read differently, pairs that
    # order them
    for entry in recorded:
        singles = {f[0]: text for e, f, text in GOLDEN if e == entry and len(f) == 1}
        pairs = [f for e, f, _ in GOLDEN if e == entry and len(f) == 2]
        keys = dict(rc.faults_of(entry))
        orderable = any(singles[a] != singles[b] and not keys[a] & keys[b] for a in singles for b in singles)
        assert singles and bool(pairs) == orderable, entry
    assert len({(e, tuple(f)) for e, f, _ in GOLDEN}) == len(GOLDEN) == 2939


def test_every_refusal_reads_as_recorded(monkeypatch):
    from libflagstats_amd import _lib
    real_lib = _lib.lib
    real_lib()

    def boom():
        raise rc.LibraryTouched()

    replayed, wrong = 0, []
    for entry, faults, want in GOLDEN:
        monkeypatch.setattr(_lib, "lib", real_lib if entry.startswith("c:") else boom)
        try:
            got = rc.message(entry, faults)
        except rc.LibraryTouched:
            got = "(not refused: the library was reached)"
        replayed += 1
        if got != want:
            wrong.append((entry, faults, got, want))
    assert not wrong, "%d of %d differ, the first: %r" % (len(wrong), replayed, wrong[:3])
    assert replayed == len(GOLDEN)


@pytest.mark.parametrize("literal", ["\"elem_bytes must be 4 or 8\"", "must be a 16-bit FLAG mask (at most 0xFFFF)", "\"min_mapq must be at most 255",
                                     "\"sel_bits must be 1 ", "\"sel_offset + n is not an index", "\"n * elem_bytes is not a size",
                                     "\"NULL mapq with min_mapq > 0 and n > 0", "\"flags: bit 0 store", "\"NULL array with n > 0"])
def test_each_rule_of_the_c_entries_is_stated_once(literal):
    """the fifteen derived units compose flagstat_derived_host.h's rules: the text of a rule stands there and nowhere else"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libflagstats_amd", "csrc")
    holders = {}
    for fn in sorted(os.listdir(csrc)):
        if fn.startswith(("flagstat_wide", "flagstat_where", "flagstat_filter", "flagstat_segments", "flagstat_derived_host")) and \
                fn.endswith((".hip", ".h")) and not fn.endswith("_device.h"):
            n = open(os.path.join(csrc, fn)).read().count(literal)
            if n:
                holders[fn] = n
    want = 2 if literal.startswith("must be a 16-bit") else 1   # require and exclude
    assert holders == {"flagstat_derived_host.h": want}, holders
