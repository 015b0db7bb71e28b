"""The two GPU block decoders are byte-exact functions, and this file checks them as such: the decode kernels are launched
directly (fsk_lz4_decode: the workgroup pipeline and the wave-per-block kernel; fsk_zstd_decode), the decoded buffer is
downloaded and compared BYTE FOR BYTE with what the image's liblz4 / libzstd decode from the same payload -- the calls
the reference makes (benchmark/flagstats.cpp:316 LZ4_decompress_safe, :96 ZSTD_decompress).  The block-file tests
(test_gpu_blockfile.py, test_gpu_zstd.py) see the decoders only through the 19 flagstat counters, which no permutation
of the flags changes and which never look at input bits 4, 5, 12-15 (libflagstats.h:118-142); here a match copied from
one flag too early, two swapped literal runs or one wrong bit anywhere fails.  The positional popcount of all 16 bits
(FLAGSTATS_hip_device_pospopcnt_u16; rule of STORM_pospopcnt_u16, python/libalgebra.h:566-574) runs on the decoded
device buffer as well: it does see bits 4, 5, 12-15."""
import os
import random
import struct

import numpy as np
import pytest

import decode_bytes_util as du
import test_gpu_blockfile as tb
from decode_bytes_util import bt

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blockfiles")
LZ4_KERNELS = [pytest.param(0, id="workgroup_kernel"), pytest.param(1, id="r03_wave_kernel")]


def run_and_compare(hip, codec, parts, what, kernel=0, ref=None, popcnt_every=1):
    """parts: [(payload, decoded size)]; every block must decode to the reference decoder's bytes"""
    ref = ref or (du.ref_zstd if codec == "zstd" else du.ref_lz4)
    wants = [ref(p, sz) for p, sz in parts]
    for i, w in enumerate(wants):
        assert w is not None, (what, i, "the reference decoder rejects this payload")
    with du.DeviceDecode(hip, codec, [p for p, _ in parts], [sz for _, sz in parts], kernel) as dd:
        for i, w in enumerate(wants):
            du.check_decoded(dd, i, w, what)
            if popcnt_every and i % popcnt_every == 0:
                assert np.array_equal(dd.pospopcnt(i), du.pospopcnt_ref(w)), (what, i, "pospopcnt of the decoded device buffer")
    return wants


def lz4_case_image(case):
    import oracle
    kw = dict(block_bytes=bt.BLOCK_BYTES, mode="fast", level=2)
    if case == "na_ragged":
        flags = oracle.generate(oracle.GEN_NA12878, 1, 1, 0, 512000 * 3 + 12345)
    elif case == "exact_multiple":      # the reference writer's trailing empty block
        flags = oracle.generate(oracle.GEN_NA12878, 2, 0, 0, 512000 * 2)
    elif case == "uniform_incompressible":
        flags = oracle.generate(oracle.GEN_UNIFORM, 3, 0xFFFF, 0, 512000 * 2 + 77)
    elif case == "hc9":
        flags = oracle.generate(oracle.GEN_NA12878, 4, 1, 0, 512000 * 2 + 999)
        kw.update(mode="hc", level=9)
    elif case == "tiny_odd_blocks":     # odd block size: the last byte of every block is no flag
        flags = oracle.generate(oracle.GEN_UNIFORM, 5, 0x0FFF, 0, 200000)
        kw.update(block_bytes=9999)
    elif case == "full_range_hc":       # every one of the 16 input bits in use, compressible: bits 4, 5, 12-15 are decoded too
        rs = np.random.RandomState(9)
        flags = np.resize(rs.randint(0, 65536, 3000).astype(np.uint16), 512000 * 2 + 31)
        flags[rs.randint(0, flags.size, 4000)] ^= np.uint16(0xF030)
        kw.update(mode="hc", level=6)
    else:                               # many_blocks
        flags = oracle.generate(oracle.GEN_NA12878, 6, 1, 0, 512000 * 40 + 5)
    return bt.block_file_image(flags, **kw), flags, kw["block_bytes"]


@pytest.mark.parametrize("kernel", LZ4_KERNELS)
@pytest.mark.parametrize("case", ["na_ragged", "exact_multiple", "uniform_incompressible", "hc9", "tiny_odd_blocks", "full_range_hc", "many_blocks"])
def test_lz4_decode_is_byte_exact_on_liblz4_written_block_files(hip, kernel, case):
    img, flags, block_bytes = lz4_case_image(case)
    parts = du.split_image(img)
    wants = run_and_compare(hip, "lz4", parts, case, kernel, popcnt_every=7 if case == "many_blocks" else 1)
    assert b"".join(wants) == flags.tobytes()       # ... and liblz4's bytes are the flags that were written


@pytest.mark.parametrize("kernel", LZ4_KERNELS)
def test_lz4_decode_is_byte_exact_on_reference_written_files(hip, kernel):
    """every .lz4 file the reference's own `bench compress` wrote (tests/golden/blockfiles, LZ4-fast and LZ4-HC)"""
    from conftest import load_golden
    names = [n for n in load_golden("blockfiles/manifest.json")["files"] if n.endswith(".lz4")]
    assert len(names) >= 3
    for name in names:
        parts = du.split_image(open(os.path.join(GOLD, name), "rb").read())
        run_and_compare(hip, "lz4", parts, name, kernel)


@pytest.mark.parametrize("kernel", LZ4_KERNELS)
@pytest.mark.parametrize("style,seed", [("bare", 1), ("bare", 2), ("edges", 3), ("edges", 4), ("mixed", 5), ("mixed", 6)])
def test_lz4_decode_is_byte_exact_on_synthetic_edge_streams(hip, kernel, style, seed):
    """valid LZ4 that liblz4 would never write (offsets around every internal boundary, self-overlapping matches, length
    bytes): against liblz4's decode AND the bytes the generator itself produced"""
    rs = np.random.RandomState(seed)
    parts, decs = [], []
    for target in [40, 300, 5000, 70000, 200000, 1 << 20, 3000, 17]:
        comp, dec = tb._synthetic_lz4_block(rs, target, style)
        parts.append((comp, len(dec)))
        decs.append(dec)
    assert run_and_compare(hip, "lz4", parts, (style, seed), kernel) == decs


@pytest.mark.parametrize("kernel", LZ4_KERNELS)
@pytest.mark.parametrize("kind", ["zeros", "period", "runs", "repeats"])
def test_lz4_decode_is_byte_exact_on_long_matches_and_literal_runs(hip, kernel, kind):
    parts, raws = [], []
    for mode, level in [("fast", 1), ("fast", 9), ("hc", 4), ("hc", 12)]:
        for i, (n, block_bytes) in enumerate([(700_001, bt.BLOCK_BYTES), (300_000, 65536), (120_003, 4096), (1_600_000, bt.BLOCK_BYTES)]):
            flags = tb._stress_flags(kind, n, 1000 * level + i)
            got = du.split_image(bt.block_file_image(flags, block_bytes=block_bytes, mode=mode, level=level))
            parts += got
            raws.append((len(got), flags.tobytes()))
    wants = run_and_compare(hip, "lz4", parts, kind, kernel, popcnt_every=5)
    at = 0
    for nblk, raw in raws:
        assert b"".join(wants[at:at + nblk]) == raw
        at += nblk


_LZ4_SEEDS = {}      # the generator is a Python loop per sequence (~0.2 s a seed): both kernels of a run share what it made


def _lz4_fuzz_seed(seed):
    """tests/perf/fuzz_lz4_gpu.py's generator: five synthetic blocks and one damaged payload per seed"""
    if seed not in _LZ4_SEEDS:
        if len(_LZ4_SEEDS) >= 320:
            _LZ4_SEEDS.clear()
        _LZ4_SEEDS[seed] = _lz4_fuzz_seed_make(seed)
    return _LZ4_SEEDS[seed]


def _lz4_fuzz_seed_make(seed):
    rs = np.random.RandomState(seed)
    style = ("bare", "edges", "mixed")[seed % 3]
    parts, decs = [], []
    for target in rs.choice([17, 100, 2000, 9000, 40000, 150000, 600000], size=5):
        comp, dec = tb._synthetic_lz4_block(rs, int(target), style)
        parts.append((comp, len(dec)))
        decs.append(dec)
    comp, n = parts[int(rs.randint(len(parts)))]
    bad = bytearray(comp)
    for _ in range(int(rs.randint(1, 6))):
        bad[int(rs.randint(len(bad)))] ^= int(rs.randint(1, 256))
    return parts, decs, (bytes(bad), n)


def lz4_fuzz_slice(hip, kernel, first, count, batch=50):
    """returns (blocks exact, damaged: both accept / both reject / GPU stricter); raises on any difference"""
    exact = both_ok = both_bad = strict = 0
    for s0 in range(first, first + count, batch):
        parts, decs, damaged = [], [], []
        for seed in range(s0, min(s0 + batch, first + count)):
            p, d, bad = _lz4_fuzz_seed(seed)
            parts += p
            decs += d
            damaged.append(bad)
        assert run_and_compare(hip, "lz4", parts, ("fuzz seeds from", s0), kernel, popcnt_every=25) == decs
        exact += len(parts)
        # damaged payloads: never more lenient than liblz4, and the same bytes when both accept
        with du.DeviceDecode(hip, "lz4", [p for p, _ in damaged], [n for _, n in damaged], kernel) as dd:
            for i, (p, n) in enumerate(damaged):
                want = du.ref_lz4(p, n)
                if dd.status[i] == 0:
                    assert want is not None, ("seed", s0 + i, "liblz4 rejects, the GPU decoder accepts")
                    du.check_decoded(dd, i, want, ("damaged, seed", s0 + i))
                    both_ok += 1
                elif want is None:
                    both_bad += 1
                else:
                    strict += 1
    return exact, both_ok, both_bad, strict


@pytest.mark.parametrize("kernel", LZ4_KERNELS)
def test_lz4_decode_is_byte_exact_on_a_slice_of_the_fuzzer(hip, kernel):
    exact, both_ok, both_bad, strict = lz4_fuzz_slice(hip, kernel, 1000, 300)
    assert exact == 1500 and both_ok + both_bad + strict == 300 and both_bad > 50
    # (the GPU decoder may refuse a damaged payload that liblz4 still decodes -- the product's own host decoder is the
    # yardstick for that in tests/perf/fuzz_lz4_gpu.py -- but a valid stream is never refused: the 1500 blocks above)
    assert strict <= 30, strict


# ------------------------------------------------------------------------------------- LZ4: blocks no compressor writes
# Everything above came out of liblz4's compressors or out of a generator that draws sequences at random.  The blocks below are
# written by tests/lz4_block_writer.py from a description (tests/test_lz4_writer_host.py holds that writer against liblz4 on the
# CPU and proves every placement): tokens, matches and literal runs ON the workgroup kernel's boundaries -- segment positions, tile
# ends, the input ring's end, the 384-byte span, 256-byte chunks, the 67,584-byte ring -- and on the wave kernel's.  The contract is
# strict: status 0, liblz4's bytes, which are the writer's, nothing behind the even length, pospopcnt of the decoded buffer.
LZ4_FAMILIES = ["segments", "stops", "literals", "span", "chunks", "tails", "ends", "wave"]


def run_placed(hip, kernel, cases, what, batch=64):
    """cases: (name, compressed, decoded, ...) from the test-only writer; a failing launch names its blocks"""
    for at in range(0, len(cases), batch):
        part = cases[at:at + batch]
        names = [c[0] for c in part]
        try:
            wants = run_and_compare(hip, "lz4", [(c[1], len(c[2])) for c in part], what, kernel)
        except AssertionError as e:
            i = next((a for a in e.args[0] if isinstance(a, int)), None) if e.args and isinstance(e.args[0], tuple) else None
            raise AssertionError("%s (blocks of this launch: %s)%s" % (e, names, "" if i is None else " -- block: " + names[i]))
        for name, want, c in zip(names, wants, part):
            assert want == c[2], (name, "liblz4's bytes are not the writer's")


@pytest.mark.parametrize("kernel", LZ4_KERNELS)
@pytest.mark.parametrize("family", LZ4_FAMILIES)
def test_lz4_decode_is_byte_exact_on_hand_placed_blocks(hip, kernel, family):
    """window-form sequences of every input length at every position of a segment, across tile ends and the input ring's end; every
    kind of token the walker hands to the scalar code; literal runs of every form, on ring byte 67,583; windows of 383..385 and of
    4,368 output bytes; matches on chunk borders, periods 1..7 over many chunks, chains inside a chunk, offsets 65,535 round the ring;
    sizes round every flush; the tightest endings liblz4 accepts; the wave kernel's own numbers.  Both kernels take every family."""
    import lz4_block_writer as bw
    assert list(bw.FAMILIES) == LZ4_FAMILIES
    run_placed(hip, kernel, bw.FAMILIES[family](), ("hand-placed", family))


@pytest.mark.parametrize("kernel", LZ4_KERNELS)
def test_lz4_decode_refuses_hand_damaged_blocks(hip, kernel):
    """one defect each -- offset 0, an offset one beyond the output, length bytes past the input, a run or a match past the declared
    size, a size one off, a cut at each of the last 20 bytes, and the three endings liblz4 refuses (a block that ends in a match,
    fewer than 5 last literals behind a match, a last match within 12 bytes of the end): a status that is not 0 for each (which
    one is not asserted: where several waves fail, the last code stands), and the valid neighbours of the same launch are exact"""
    import lz4_block_writer as bw
    bad = bw.rejected()
    good = [c for c in bw.FAMILIES["tails"]() if len(c[2]) < 70000][:len(bad) + 1]
    good = (good * (len(bad) // len(good) + 2))[:len(bad) + 1]
    payloads, sizes = [good[0][1]], [len(good[0][2])]
    for (name, comp, usize), g in zip(bad, good[1:]):
        payloads += [comp, g[1]]
        sizes += [usize, len(g[2])]
    accepted = []
    with du.DeviceDecode(hip, "lz4", payloads, sizes, kernel) as dd:
        for i, (name, comp, usize) in enumerate(bad):
            st = int(dd.status[2 * i + 1])
            print("kernel %d: status %2d  %s" % (kernel, st, name))
            if st == 0:
                accepted.append(name)
        for i, g in enumerate(good):
            du.check_decoded(dd, 2 * i, g[2], ("the valid neighbour", g[0], "before", bad[i][0] if i < len(bad) else None))
    assert not accepted, ("damaged blocks the GPU decoder accepts", accepted)


def lz4_shape_fuzz_slice(hip, kernel, first, count, batch=50):
    """lz4_block_writer.random_block over a seed range: every block exact, two damaged variants per block under the rule of
    lz4_fuzz_slice; returns (exact, both accept, both reject, GPU stricter)"""
    import lz4_block_writer as bw
    exact = both_ok = both_bad = strict = 0
    for s0 in range(first, first + count, batch):
        cases, damaged = [], []
        for seed in range(s0, min(s0 + batch, first + count)):
            rng = random.Random(seed)
            comp, dec, layout = bw.random_block(rng)
            cases.append(("shape fuzz seed %d" % seed, comp, dec))
            for _ in range(2):
                bad = bytearray(comp)
                for _ in range(rng.randint(1, 5)):
                    bad[rng.randrange(len(bad))] ^= rng.randint(1, 255)
                damaged.append((bytes(bad) if rng.random() < 0.8 else bytes(bad[:rng.randrange(1, len(bad) + 1)]), len(dec)))
        run_placed(hip, kernel, cases, ("shape fuzz seeds from", s0), batch=batch)
        exact += len(cases)
        with du.DeviceDecode(hip, "lz4", [p for p, _ in damaged], [n for _, n in damaged], kernel) as dd:
            for i, (p, n) in enumerate(damaged):
                want = du.ref_lz4(p, n)
                if dd.status[i] == 0:
                    assert want is not None, ("seed", s0 + i // 2, "liblz4 rejects, the GPU decoder accepts")
                    du.check_decoded(dd, i, want, ("damaged, seed", s0 + i // 2))
                    both_ok += 1
                elif want is None:
                    both_bad += 1
                else:
                    strict += 1
    return exact, both_ok, both_bad, strict


@pytest.mark.parametrize("kernel", LZ4_KERNELS)
def test_lz4_decode_is_byte_exact_on_a_slice_of_the_placed_fuzzer(hip, kernel):
    exact, both_ok, both_bad, strict = lz4_shape_fuzz_slice(hip, kernel, 0, 300)
    print("placed fuzz, kernel %d: %d exact; damaged: both accept %d, both reject %d, GPU stricter %d" % (kernel, exact, both_ok, both_bad, strict))
    assert exact == 300 and both_ok + both_bad + strict == 600


# ------------------------------------------------------------------------------------------------------------ Zstandard
def _zstd_parts(raws, level):
    return [(bt.compress_block(raw, "zstd", level), len(raw)) for raw in raws]


@pytest.mark.parametrize("level", [1, 5, 12, 19, -5])
def test_zstd_decode_is_byte_exact_on_synthetic_streams(hip, level):
    """raw / RLE / compressed blocks, eleven-block frames, four Huffman streams, runs above 16,383, matches at distances
    around the 32 KiB ring, the old 64 KiB one and the block size (test_gpu_zstd.synthetic_blocks)"""
    from test_gpu_zstd import synthetic_blocks
    raws = synthetic_blocks(100 + abs(level))
    assert run_and_compare(hip, "zstd", _zstd_parts(raws, level), ("synthetic", level)) == raws


def test_zstd_decode_is_byte_exact_on_reference_written_files(hip):
    from conftest import load_golden
    man = load_golden("blockfiles/manifest.json")["files"]
    names = [n for n, e in man.items() if e.get("codec") == "zstd"]
    assert len(names) >= 3
    for name in names:
        run_and_compare(hip, "zstd", du.split_image(open(os.path.join(GOLD, name), "rb").read()), name)


@pytest.mark.parametrize("level", [1, 3, 9, 19, -5])
def test_zstd_decode_is_byte_exact_on_block_files(hip, level):
    import oracle
    flags = oracle.generate(oracle.GEN_NA12878, 30 + abs(level), 1, 0, 512000 * 3 + 12345)
    parts = du.split_image(bt.block_file_image(flags, mode="zstd", level=level))
    assert b"".join(run_and_compare(hip, "zstd", parts, ("na", level))) == flags.tobytes()
    # every input bit in use, still compressible
    rs = np.random.RandomState(level + 50)
    full = np.resize(rs.randint(0, 65536, 5000).astype(np.uint16), 512000 + 77)
    full[rs.randint(0, full.size, 3000)] ^= np.uint16(0xF030)
    parts = du.split_image(bt.block_file_image(full, mode="zstd", level=level))
    assert b"".join(run_and_compare(hip, "zstd", parts, ("full range", level))) == full.tobytes()


@pytest.mark.parametrize("block_bytes", [9999, 70001, 4096000])
def test_zstd_decode_is_byte_exact_on_other_block_sizes(hip, block_bytes):
    import oracle
    flags = oracle.generate(oracle.GEN_NA12878, 51, 1, 0, 2048000 * 2 + 333)
    parts = du.split_image(bt.block_file_image(flags, block_bytes=block_bytes, mode="zstd", level=2))
    assert b"".join(run_and_compare(hip, "zstd", parts, block_bytes, popcnt_every=50)) == flags.tobytes()


def test_zstd_decode_is_byte_exact_on_frames_of_many_small_blocks(hip):
    """35 blocks in a frame: taken at once, byte-exact.  52 blocks, 391 blocks (a 1 KiB window), 1000 blocks: the first-pass entry
    answers "too many blocks" (never a wrong byte), the second-pass entry (fsk_zstd_decode_ex: a block slot per KiB) decodes them
    byte for byte."""
    import ctypes

    import oracle
    from zstd_fuzz_gen import flushed_frame
    z = bt.zstd()
    raw = oracle.generate(oracle.GEN_NA12878, 77, 1, 0, 512000).tobytes()
    run_and_compare(hip, "zstd", [(flushed_frame(z, raw, 30000), len(raw)), (flushed_frame(z, raw[:300001], 9000), 300001)], "35 blocks")
    # ZSTD_compress2 with windowLog 10: blocks of 1 KiB
    z.ZSTD_createCCtx.restype = ctypes.c_void_p
    z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
    z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    z.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    z.ZSTD_compress2.restype = ctypes.c_size_t
    cctx = z.ZSTD_createCCtx()
    z.ZSTD_CCtx_setParameter(cctx, 101, 10)          # ZSTD_c_windowLog
    small = raw[:400000]
    dst = ctypes.create_string_buffer(z.ZSTD_compressBound(len(small)))
    n = z.ZSTD_compress2(cctx, dst, len(dst), small, len(small))
    z.ZSTD_freeCCtx(cctx)
    assert not z.ZSTD_isError(n)
    cases = [("52 blocks", flushed_frame(z, raw, 20000), raw), ("1 KiB window", dst.raw[:n], small), ("1000 blocks", flushed_frame(z, raw, 1024), raw)]
    for what, frame, want in cases:
        assert du.ref_zstd(frame, len(want)) == want
        with du.DeviceDecode(hip, "zstd", [frame], [len(want)]) as dd:
            if dd.status[0] == 0:
                du.check_decoded(dd, 0, want, what)
            else:
                assert dd.status[0] == 67, (what, int(dd.status[0]))       # kZstdTooManyBlocks
        with du.DeviceDecode(hip, "zstd", [frame], [len(want)], min_blocks=len(want) // 1024 + 16) as dd:
            du.check_decoded(dd, 0, want, what + ", second pass")
            assert np.array_equal(dd.pospopcnt(0), du.pospopcnt_ref(want))


def zstd_fuzz_slice(hip, first, count, batch=50):
    """tests/perf/fuzz_zstd_gpu.py's generator (a third of the frames from ZSTD_compress2 with random advanced parameters),
    three damaged variants per frame; returns (exact, not taken, both accept, both reject, GPU stricter)"""
    from zstd_fuzz_gen import compress_with_parameters, damage, synthetic
    z = bt.zstd()
    exact = untaken = both_ok = both_bad = strict = 0
    for s0 in range(first, first + count, batch):
        parts, raws, damaged = [], [], []
        for seed in range(s0, min(s0 + batch, first + count)):
            rng = random.Random(seed)
            raw = synthetic(rng, np.random.default_rng(seed))
            level = rng.choice([1, 1, 2, 3, 5, 7, 9, 12, 15, 19, -1, -5])
            comp = compress_with_parameters(z, rng, raw) if seed % 3 == 2 else None
            if comp is None:
                comp = bt.compress_block(raw, "zstd", level)
            parts.append((comp, len(raw)))
            raws.append(raw)
            damaged += [(damage(rng, comp), len(raw)) for _ in range(3)]
        with du.DeviceDecode(hip, "zstd", [p for p, _ in parts], [n for _, n in parts]) as dd:
            for i, raw in enumerate(raws):
                assert du.ref_zstd(parts[i][0], len(raw)) == raw
                if 64 <= dd.status[i] < du.NOT_RUN:
                    untaken += 1         # valid Zstandard the decoder does not take (a window of a few KiB: hundreds of blocks)
                    continue
                du.check_decoded(dd, i, raw, ("fuzz seed", s0 + i))
                if i % 10 == 0:
                    assert np.array_equal(dd.pospopcnt(i), du.pospopcnt_ref(raw)), ("fuzz seed", s0 + i)
                exact += 1
        with du.DeviceDecode(hip, "zstd", [p for p, _ in damaged], [n for _, n in damaged]) as dd:
            for i, (p, n) in enumerate(damaged):
                want = du.ref_zstd(p, n)
                if dd.status[i] == 0:
                    assert want is not None, ("seed", s0 + i // 3, "libzstd rejects, the GPU decoder accepts")
                    du.check_decoded(dd, i, want, ("damaged, seed", s0 + i // 3))
                    both_ok += 1
                elif want is None:
                    both_bad += 1
                else:
                    strict += 1
    return exact, untaken, both_ok, both_bad, strict


def test_zstd_decode_is_byte_exact_on_a_slice_of_the_fuzzer(hip):
    exact, untaken, both_ok, both_bad, strict = zstd_fuzz_slice(hip, 0, 300)
    assert exact + untaken == 300 and exact >= 270, (exact, untaken)
    assert both_ok + both_bad + strict == 900 and both_bad > 300


# ----------------------------------------------------------------------------- Zstandard: frames no compressor writes
# Everything above came out of libzstd's compressor, so it has the forms, lengths and distances that compressor chooses.  The
# frames below are written by tests/zstd_frame_writer.py from a description (tests/test_zstd_writer_host.py holds that writer
# against libzstd on the CPU): every form of the format, and exact numbers on the execution kernel's own boundaries.  The
# contract is strict: status 0 and libzstd's bytes, which are the writer's; no "not taken" code, these forms are not on the
# list of exceptions in flagstat_zstd_kernels.h.
def run_written(hip, frames, what, batch=48):
    """frames: (name, frame, decoded bytes) from the test-only writer"""
    for at in range(0, len(frames), batch):
        part = frames[at:at + batch]
        names = [name for name, _, _ in part]
        try:
            wants = run_and_compare(hip, "zstd", [(f, len(w)) for _, f, w in part], what, popcnt_every=3)
        except AssertionError as e:
            i = next((a for a in e.args[0] if isinstance(a, int)), None) if e.args and isinstance(e.args[0], tuple) else None
            raise AssertionError("%s (frames of this launch: %s)%s" % (e, names, "" if i is None else " -- frame: " + names[i]))
        for name, want, (_, _, own) in zip(names, wants, part):
            assert want == own, (name, "libzstd's bytes are not the writer's")


@pytest.mark.parametrize("family", ["header", "literals", "huffman", "sequences", "tables", "repeats", "mixed"])
def test_zstd_decode_is_byte_exact_on_hand_written_forms(hip, family):
    """header forms; literals raw / RLE / Huffman / treeless in every size format, one stream and four; Huffman trees of depth 1..11
    as direct and as FSE-compressed weights; sequence counts in one, two and three bytes; predefined, RLE, FSE (every accuracy
    log) and repeat mode for each table; the six repeat-offset cases from a known and from a carried history; frames of twelve
    blocks that mix them"""
    import zstd_frame_writer as fw
    assert list(fw.FAMILIES) == ["header", "literals", "huffman", "sequences", "tables", "repeats", "mixed"]
    run_written(hip, fw.FAMILIES[family](), ("hand-written", family))


@pytest.mark.parametrize("family", ["runs", "near", "far", "huge", "seams", "boundaries", "dense", "literal_use"])
def test_zstd_decode_is_byte_exact_on_the_kernels_own_boundaries(hip, family):
    """literal runs and matches of k * 16383 + {-1, 0, 1}, 65535, 65536 and a whole block; offsets 1..8 round the ring; offsets at
    the ring's reach (32 KiB), its size (36 KiB), 64 KiB, 128 KiB, 256 KiB; 3 MiB reaching back to the first byte; sources that end at,
    before and behind the start of the record that copies them; matches and literal runs across blocks; the densest bit
    streams the format has; all literals used and none.  (Blocks of 63..65, 127..129 and 0x7EFF..0x7F01 sequences: "sequences" above.)"""
    import zstd_frame_writer as fw
    assert list(fw.GEOMETRY) == ["runs", "near", "far", "huge", "seams", "boundaries", "dense", "literal_use"]
    run_written(hip, fw.GEOMETRY[family](), ("geometry", family), batch=24)


def test_zstd_decode_declines_valid_frames_beyond_its_limits_by_name(hip):
    """Valid Zstandard that flagstat_zstd_kernels.h says the decoder does not take -- a content checksum, a dictionary ID field,
    a skippable frame in front, a second frame behind, more than 64 MiB: libzstd decodes each, the decoder answers with the code
    for it.  Where two limits apply (64 MiB + 2 bytes in 513 RLE blocks: too large, and too many blocks) either code is right.
    Never status 0 with other bytes, never a damage code (1..63)."""
    import zstd_frame_writer as fw
    seen = set()
    for name, frame, want, codes in fw.limit_frames():
        assert du.ref_zstd(frame, len(want)) == want, name
        with du.DeviceDecode(hip, "zstd", [frame], [len(want)]) as dd:
            st = int(dd.status[0])
            print("%s: status %d" % (name, st))
            if st == 0:
                du.check_decoded(dd, 0, want, name)
            assert st in codes, (name, st, "allowed", codes)
            seen.add(st)
    assert {64, 65, 66, 68} <= seen and seen & {67, 69}


def test_zstd_decode_takes_a_hand_written_frame_of_many_blocks_in_the_second_pass(hip):
    """60 small blocks of every kind, trees, tables and offset history carried from block to block: the first-pass entry may answer
    "too many blocks" (12 slots for a frame this small), never wrong bytes; with a slot per block it decodes them byte for byte"""
    import zstd_frame_writer as fw
    rng = random.Random(5)
    abc = bytes(rng.sample(range(129), 30))
    w = fw.FrameWriter().raw(rng.randbytes(500))
    w.compressed(bytes(rng.choices(abc, k=400)), [(3, 9, 100), (0, 4, 7)], lit="huf", streams=4, tree=fw.tree_for(abc, 7, rng), describe="fse",
                 modes=("fse", "fse", "fse"), logs=(9, 8, 9), low=fw.EVERY_CODE)
    for k in range(58):
        if k % 7 == 3:
            w.raw(rng.randbytes(k))
        elif k % 7 == 5:
            w.rle(k, 100 * k)
        else:
            seqs = [(rng.randrange(1, 4), rng.randrange(3, 30), rng.choice([-1, -2, -3, rng.randrange(1, 500)])) for _ in range(1 + k % 5 * 20)]
            w.compressed(bytes(rng.choices(abc, k=sum(s[0] for s in seqs) + 8)), seqs, lit=("treeless", "huf")[k % 11 == 0], tree=fw.tree_for(abc, 5 + k % 6, rng),
                         describe=("direct", "fse")[k % 2], streams=(1, 4)[k % 2], modes=(("repeat",) * 3, ("repeat", "predef", "fse"))[k % 4 == 0], low=fw.EVERY_CODE)
    frame, want = w.finish()
    assert len(w.body) == 60 and du.ref_zstd(frame, len(want)) == want
    with du.DeviceDecode(hip, "zstd", [frame], [len(want)]) as dd:
        if dd.status[0] == 0:
            du.check_decoded(dd, 0, want, "60 blocks")
        else:
            assert dd.status[0] == 67, int(dd.status[0])
    with du.DeviceDecode(hip, "zstd", [frame], [len(want)], min_blocks=64) as dd:
        du.check_decoded(dd, 0, want, "60 blocks, second pass")
        assert np.array_equal(dd.pospopcnt(0), du.pospopcnt_ref(want))


def zstd_shape_fuzz_slice(hip, first, count, batch=50):
    """zstd_frame_writer.random_frame over a seed range: every frame exact (no "not taken": at most 12 blocks each), two damaged
    variants per frame under the rule of zstd_fuzz_slice; returns (exact, both accept, both reject, GPU stricter)"""
    import zstd_frame_writer as fw
    from zstd_fuzz_gen import damage
    exact = both_ok = both_bad = strict = 0
    for s0 in range(first, first + count, batch):
        frames, damaged = [], []
        for seed in range(s0, min(s0 + batch, first + count)):
            rng = random.Random(seed)
            frame, want = fw.random_frame(rng)
            frames.append(("shape fuzz seed %d" % seed, frame, want))
            damaged += [(damage(rng, frame), len(want)) for _ in range(2)]
        run_written(hip, frames, ("shape fuzz seeds from", s0), batch=batch)
        exact += len(frames)
        with du.DeviceDecode(hip, "zstd", [p for p, _ in damaged], [n for _, n in damaged]) as dd:
            for i, (p, n) in enumerate(damaged):
                want = du.ref_zstd(p, n)
                if dd.status[i] == 0:
                    assert want is not None, ("seed", s0 + i // 2, "libzstd rejects, the GPU decoder accepts")
                    du.check_decoded(dd, i, want, ("damaged, seed", s0 + i // 2))
                    both_ok += 1
                elif want is None:
                    both_bad += 1
                else:
                    strict += 1
    return exact, both_ok, both_bad, strict


def test_zstd_decode_is_byte_exact_on_a_slice_of_the_shape_fuzzer(hip):
    exact, both_ok, both_bad, strict = zstd_shape_fuzz_slice(hip, 0, 300)
    print("shape fuzz: %d exact; damaged: both accept %d, both reject %d, GPU stricter %d" % (exact, both_ok, both_bad, strict))
    assert exact == 300 and both_ok + both_bad + strict == 600


def test_decoders_write_nothing_outside_their_blocks(hip):
    """Blocks of every length mod 16 packed back to back in 16-byte slots: each slot's slack (and an odd last byte) still
    holds the fill pattern after the launch -- a decoder that stores a vector too far would hit its neighbour."""
    rs = np.random.RandomState(4)
    raws = []
    for n in list(range(0, 40)) + [1023, 1024, 1025, 4095, 4097, 65535, 65537, 131071, 131073]:
        a = np.resize(rs.randint(0, 4096, max(1, n // 7 + 1)).astype(np.uint16), (n + 1) // 2).tobytes()[:n]
        raws.append(a)
    for kernel in (0, 1):
        run_and_compare(hip, "lz4", [(bt.compress_block(r, "fast", 1), len(r)) for r in raws], ("slots", kernel), kernel)
    run_and_compare(hip, "zstd", _zstd_parts(raws, 3), "slots")
