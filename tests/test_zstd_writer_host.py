"""The test-only Zstandard frame writer (tests/zstd_frame_writer.py) held against libzstd, and the two Python restatements of the
GPU decoder (tests/zstd_model.py: RFC 8878; tests/zstd_gpu_model.py: the kernels' records and bit arithmetic) held against the
writer's frames -- valid Zstandard of every form the format has, which no compressor writes.  No GPU: what these tests prove is
that the frames the GPU tests feed the decoder (tests/test_gpu_decode_bytes.py, tests/test_gpu_zstd.py) are what they claim to be,
that the census below reaches every form, and that the model the kernels were written against decodes them.
The reference decodes every payload with ZSTD_decompress (benchmark/flagstats.cpp:636-682): that call is the yardstick here."""
import ctypes
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import blockfile_tool as bt  # noqa: E402
import zstd_frame_writer as fw  # noqa: E402
import zstd_gpu_model as gm  # noqa: E402
import zstd_model as zm  # noqa: E402

try:
    Z = bt.zstd()
except OSError:  # pragma: no cover
    Z = None
pytestmark = pytest.mark.skipif(Z is None, reason="no libzstd.so.1")

FUZZ_SEEDS = range(0, 60)       # set by time: a seed costs a quarter of a second here, nearly all of it the two Python decoders

# Every form of the format the GPU decoder implements.  The hand-written corpus (zstd_frame_writer.form_corpus) must reach each
# in at least three different frames; a decoder feature added later gets its line here and its frames there.
FORMS = [
    # frame header: single segment or window descriptor, content size absent or in 1, 2, 4, 8 bytes
    "hdr single fcs1", "hdr single fcs2", "hdr single fcs4", "hdr single fcs8",
    "hdr window fcs0", "hdr window fcs2", "hdr window fcs4", "hdr window fcs8",
    "block raw", "block rle", "block compressed",
    # literals section: raw and RLE in their three size formats, Huffman-coded with a tree or without, one stream or four
    "lit raw 1B", "lit raw 2B", "lit raw 3B", "lit rle 1B", "lit rle 2B", "lit rle 3B",
    "lit huf 1 stream", "lit huf 4 streams 3B", "lit huf 4 streams 4B", "lit huf 4 streams 5B",
    "lit treeless 1 stream", "lit treeless 4 streams 3B", "lit treeless 4 streams 4B", "lit treeless 4 streams 5B",
    # Huffman tree description and depth
    "tree direct", "tree fse", "tree above 128 weights",
] + ["tree depth %d" % d for d in range(1, 12)] + [
    # sequence count: none, one byte, two bytes, three bytes (from 0x7F00), and where one byte becomes two
    "nseq 0", "nseq 1B", "nseq 2B", "nseq 3B", "nseq 127..129",
] + ["mode %s %s" % (t, m) for t in ("ll", "of", "ml") for m in ("predef", "rle", "fse", "repeat")] + [
    "log ll %d" % n for n in range(5, 10)] + ["log of %d" % n for n in range(5, 9)] + ["log ml %d" % n for n in range(5, 10)] + [
    # repeat offsets: codes 1..3 after literals, and shifted by one (code 3: first offset - 1) after none
    "rep code %d ll%s" % (c, z) for c in (1, 2, 3) for z in (">0", "=0")] + [
    # what a compressed block takes over from earlier ones, when the block right before it is of another kind
    "%s after %s" % (what, prev) for what in ("treeless literals", "repeat-mode table", "repeat offset")
    for prev in ("raw block", "rle block", "zero-sequence block")]

_DETAILS = {}


def zm_details(family):
    """the RFC model's decode of every frame of a family of the form corpus (asserted equal to the writer's bytes), kept for the census"""
    if family not in _DETAILS:
        out = []
        for name, frame, want in fw.FAMILIES[family]():
            det = []
            assert zm.decode_frame(frame, det) == want, name
            out.append(det)
        _DETAILS[family] = out
    return _DETAILS[family]


def check_libzstd(name, frame, want):
    assert ref_decode(frame, len(want)) == want, (name, "libzstd does not decode this frame to the writer's bytes")


def ref_decode(frame, n):
    dst = ctypes.create_string_buffer(max(n, 1))
    r = Z.ZSTD_decompress(dst, n, bytes(frame), len(frame))
    return None if Z.ZSTD_isError(r) or r != n else dst.raw[:n]


def check_gpu_model(name, frame, want):
    try:
        got = gm.decode(frame, len(want))
    except gm.Fail as f:
        raise AssertionError("%s: the GPU decoder's model answers %d for a valid frame" % (name, f.code))
    assert got == want, (name, "the GPU decoder's model decodes other bytes")


@pytest.mark.parametrize("family", list(fw.FAMILIES))
def test_form_corpus_against_libzstd_and_both_models(family):
    frames = fw.FAMILIES[family]()
    assert len({f for _, f, _ in frames}) == len(frames) and len({n for n, _, _ in frames}) == len(frames)
    for name, frame, want in frames:
        check_libzstd(name, frame, want)      # the cap is zero: a frame libzstd refuses is a writer bug
    zm_details(family)
    for name, frame, want in frames:
        check_gpu_model(name, frame, want)


@pytest.mark.parametrize("family", list(fw.GEOMETRY))
def test_geometry_corpus_against_libzstd_and_both_models(family):
    for name, frame, want in fw.GEOMETRY[family]():
        check_libzstd(name, frame, want)
        assert zm.decode_frame(frame) == want, name
        check_gpu_model(name, frame, want)


def test_limit_frames_are_valid_and_the_model_declines_them_by_name():
    """what flagstat_zstd_kernels.h lists as "valid, not taken": libzstd decodes each, the GPU decoder's model answers with the
    code for it (where the header says two limits may be met, either), never with a damage code and never with bytes"""
    seen = set()
    for name, frame, want, codes in fw.limit_frames():
        check_libzstd(name, frame, want)
        with pytest.raises(gm.Fail) as f:
            gm.decode(frame, len(want))
        assert f.value.code in codes, (name, f.value.code)
        seen.add(f.value.code)
    assert {64, 65, 66, 68} <= seen and seen & {67, 69}


def test_shape_fuzzer_against_libzstd_and_both_models():
    blocks = forms = 0
    seen = set()
    for seed in FUZZ_SEEDS:
        frame, want = fw.random_frame(random.Random(seed))
        check_libzstd(("seed", seed), frame, want)
        det = []
        assert zm.decode_frame(frame, det) == want, seed
        check_gpu_model(("seed", seed), frame, want)
        blocks += len(det)
        seen |= fw.forms_of(frame, det)
    print("\n%d seeds, %d blocks, %d of the census's %d forms" % (len(FUZZ_SEEDS), blocks, len(seen & set(FORMS)), len(FORMS)))
    assert len(seen & set(FORMS)) > len(FORMS) // 2


def census(frames_and_details):
    count = {}
    for frame, det in frames_and_details:
        for form in fw.forms_of(frame, det):
            count[form] = count.get(form, 0) + 1
    return count


def test_census_every_form_is_reached_in_three_hand_written_frames():
    assert len(set(FORMS)) == len(FORMS)
    pairs = []
    for family, make in fw.FAMILIES.items():
        pairs += [(frame, det) for (_, frame, _), det in zip(make(), zm_details(family))]
    count = census(pairs)
    print("\ncensus of the hand-written corpus, %d frames (frames per form):" % len(pairs))
    for form in FORMS:
        print("  %-48s %d" % (form, count.get(form, 0)))
    unlisted = sorted(set(count) - set(FORMS))
    assert not unlisted, ("forms_of names forms that FORMS does not list", unlisted)
    short = {f: count.get(f, 0) for f in FORMS if count.get(f, 0) < 3}
    assert not short, short


def test_census_of_what_libzstd_writes():
    """printed with -s, no assertion: what the compressor-written corpus of the GPU tests (a slice of tests/zstd_fuzz_gen.py's
    generator, as test_gpu_decode_bytes.zstd_fuzz_slice draws it) leaves out"""
    import numpy as np
    from zstd_fuzz_gen import compress_with_parameters, synthetic
    pairs = []
    for seed in range(40):
        rng = random.Random(seed)
        raw = synthetic(rng, np.random.default_rng(seed))
        level = rng.choice([1, 1, 2, 3, 5, 7, 9, 12, 15, 19, -1, -5])
        comp = compress_with_parameters(Z, rng, raw) if seed % 3 == 2 else None
        if comp is None:
            comp = bt.compress_block(raw, "zstd", level)
        if len(raw) > 140000:
            continue            # (for time: the Python decoder takes seconds for these)
        det = []
        assert zm.decode_frame(comp, det) == raw
        pairs.append((comp, det))
    count = census(pairs)
    print("\ncensus of %d frames libzstd wrote: never reached: %s" % (len(pairs), ", ".join(f for f in FORMS if f not in count)))
    print("  reached once or twice: %s" % ", ".join("%s (%d)" % (f, count[f]) for f in FORMS if 0 < count.get(f, 0) < 3))


def test_writer_parts():
    """XXH64 against published values; the FSE table description against its reader, over random counts with "less than one"
    probabilities and long runs of zeros"""
    assert fw.xxh64(b"") == 0xEF46DB3751D8E999
    assert fw.xxh64(b"a") == 0xD24EC4F1A98C6E5B
    assert fw.xxh64(b"abc") == 0x44BC2CF5AD770999
    rng = random.Random(3)
    for _ in range(400):
        log = rng.randrange(5, 10)
        nsym = rng.randrange(2, 53)
        used = rng.sample(range(nsym), rng.randrange(2, min(nsym, 1 << log) + 1))
        low = set(rng.sample(used, rng.randrange(0, len(used))))
        counts = fw.make_counts(used, log, low=low, rng=rng)
        data = fw.write_fse_counts(counts, log)
        got_log, got, end = zm.read_fse_counts(data + b"\0" * 8, 0, 52, 9)
        while counts and counts[-1] == 0:
            counts.pop()
        assert (got_log, got, end) == (log, counts, len(data))
