"""Every stream-taking device entry, and the torch layer on top of it, captured into a HIP graph with torch.cuda.graph, replayed,
its buffers rewritten, replayed again.

What a capture can get wrong that a plain launch cannot: a call that is illegal (or runs beside the capture) while the stream is
capturing; a store form whose zeroing memset is no node of the graph, so that a replay accumulates; workspace state (K1's tickets
and per-XCD copies) that a replay inherits from the replay or plain launch before it; and anything but pointers and geometry
frozen into the graph -- a replay must count what the buffers hold NOW, and knobs changed after the capture must not matter.

Every case goes through one protocol (``capture_and_replay``): a plain call first (the engine exists, as the header asks), result
words set to sentinels (bias words for the += form, garbage for the store form), ONE call captured on a fresh stream, the words
still sentinels after the capture (nothing ran beside it), three replays (+= rows: bias + 3 x want, `high` the OR; store rows:
exactly want, again after garbage was written over them), data set B copied into the same buffers and one replay (want of B),
and a plain call of the same entry on other buffers between two replays on the capture stream (both right).

Inputs and expected values come from tests/graphs_plan.py (checked without a GPU by test_graphs_plan_host.py): two data sets of
the same sizes and alignments, arrays inside slabs whose surroundings would change every result, and oracle values only.  Every
comparison is exact."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphs_plan as gp  # noqa: E402
from test_gpu_where import BIAS, GARBAGE, SEL_BIAS, STORE, SUPERSET, err, u64  # noqa: E402

pytestmark = pytest.mark.gpu

HIGH_BIAS = 1 << 50                            # a bit no element of the wide columns carries
SENTINEL = {"out": BIAS, "selected": SEL_BIAS, "high": HIGH_BIAS}
NSEG = gp.NSEG
FLAGS, GROUPED, OFFSETS, MAPQ = ("flags", "edge"), ("flags", "grouped"), "offsets", "mapq"
SEL_BYTES, SEL_BITMAP = ("sel", "bytes"), ("sel", "bitmap")
N = gp.SHAPES["edge"][0]
BOTH_MODES = (STORE | SUPERSET, 0)


@pytest.fixture(scope="module")
def plan(oracle_mod):
    return gp.plan(oracle_mod)


# ------------------------------------------------------------------ device copies, result words, knobs
def to_device(host):
    """a host array of the plan as a CUDA tensor (unsigned 16- and 64-bit elements as the signed dtype of their width)"""
    import torch
    signed = {"uint16": np.int16, "uint64": np.int64}.get(host.dtype.name)
    return torch.from_numpy(host.view(signed) if signed else host).cuda()


class Dev:
    """device copies of some of the plan's slabs, holding one of its data sets"""

    def __init__(self, plan, names, ds="A"):
        self.slabs = {name: plan.slabs[name] for name in names}
        self.t = {name: to_device(slab.host(ds)) for name, slab in self.slabs.items()}
        assert all(t.data_ptr() % 16 == 0 for t in self.t.values())

    def load(self, ds):
        """copy another data set into the same tensors"""
        import torch
        for name, slab in self.slabs.items():
            self.t[name].copy_(to_device(slab.host(ds)))
        torch.cuda.synchronize()

    def ptr(self, name):
        return self.t[name].data_ptr() + self.slabs[name].at * self.t[name].element_size()

    def view(self, name):
        slab = self.slabs[name]
        return self.t[name][slab.at:slab.at + slab.n]


class Words:
    """the result words of one call: int64 CUDA tensors by name -- "out" (counters), "selected", "high" -- in separate allocations
    or (``together``) one behind the other in a single one, as the entries' one-memset layouts want them"""

    def __init__(self, store, shapes, together=False):
        import torch
        self.store = store
        sizes = {name: int(np.prod(shape)) for name, shape in shapes.items()}
        if together:
            whole = torch.empty(sum(sizes.values()), dtype=torch.int64, device="cuda")
            starts = np.concatenate([[0], np.cumsum(list(sizes.values()))])
            self.t = {name: whole[int(b):int(b) + sizes[name]].view(shapes[name]) for name, b in zip(shapes, starts)}
            assert all(self.ptr(b) == self.ptr(a) + 8 * sizes[a] for a, b in zip(list(shapes), list(shapes)[1:]))
        else:
            self.t = {name: torch.empty(shape, dtype=torch.int64, device="cuda") for name, shape in shapes.items()}
        self.fill = {name: GARBAGE if store else SENTINEL[name] for name in shapes}
        self.reset()

    def reset(self):
        import torch
        for name, t in self.t.items():
            t.fill_(self.fill[name])
        torch.cuda.synchronize()

    def ptr(self, name):
        return self.t[name].data_ptr()

    def untouched(self, note):
        import torch
        torch.cuda.synchronize()
        for name, t in self.t.items():
            assert (u64(t) == np.uint64(self.fill[name])).all(), (note, name, "touched beside the capture", u64(t).ravel()[:8])

    def check(self, want, times, note):
        """after `times` launches over the sentinels: want in the store form, else sentinel + times x want (`high`: sentinel | want)"""
        import torch
        torch.cuda.synchronize()
        assert set(want) == set(self.t), (note, sorted(want), sorted(self.t))
        for name, t in self.t.items():
            w = np.asarray(want[name], dtype=np.uint64)
            if self.store:
                expect = w
            elif name == "high":
                expect = w | np.uint64(HIGH_BIAS)
            else:
                expect = np.uint64(self.fill[name]) + np.uint64(times) * w
            got = u64(t).reshape(w.shape)
            if not np.array_equal(got, expect):
                bad = np.nonzero(got != expect)
                raise AssertionError((note, name, "x%d" % times, "at", [b[:6] for b in bad], "got", got[bad][:6], "want", expect[bad][:6]))


@contextlib.contextmanager
def knob(hip, key, value):
    old = hip.FLAGSTATS_hip_get(key)
    try:
        assert hip.FLAGSTATS_hip_set(key, value) == 0, err(hip)
        yield
    finally:
        hip.FLAGSTATS_hip_set(key, old)
    assert hip.FLAGSTATS_hip_get(key) == old


@contextlib.contextmanager
def chain_from_one_unit(hip):
    """the segmented kernels' policy with min_units = 1: over the edge shape no wave owns two whole units, so the shipped policy
    (2) counts every segment flag by flag; with 1 the long segment's whole units go through the carry-save chain"""
    hip.fsk_segments_policy.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    hip.fsk_segments_policy.restype = None
    hip.fsk_set_segments_policy.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    hip.fsk_set_segments_policy.restype = None

    def get():
        mu, bpc = ctypes.c_uint32(), ctypes.c_uint32()
        hip.fsk_segments_policy(ctypes.byref(mu), ctypes.byref(bpc))
        return mu.value, bpc.value

    saved = get()
    try:
        hip.fsk_set_segments_policy(1, saved[1])
        assert get() == (1, saved[1])
        yield
    finally:
        hip.fsk_set_segments_policy(*saved)
    assert get() == saved


def last_mode(hip):
    hip.fsk_last_mode.restype = ctypes.c_int
    hip.fsk_last_mode.argtypes = []
    return hip.fsk_last_mode()


def raw(stream):
    return ctypes.c_void_p(stream.cuda_stream)


def wants(plan, key, superset=True, names=None):
    """{data set: {result name: uint64 array}} of a plan entry, the counters cut to the form a launch without the superset flag
    reports"""
    return {ds: {name: (gp.cut(w, superset) if name == "out" and w.shape[-1] == 32 else w)
                 for name, w in plan.want[key][ds].items() if names is None or name in names} for ds in gp.DATA_SETS}


# ------------------------------------------------------------------ the protocol
class Case:
    """one entry with its arguments.  ``launch(hip, dev, words, stream)`` queues ONE call that reads the device copies ``dev`` and
    writes the result words ``words`` on the torch stream ``stream``, and returns the entry's return code.  ``knobs``: context
    managers (taking hip) that hold around the CAPTURE only; ``mode``: what fsk_last_mode must read after the capturing call."""

    def __init__(self, note, inputs, store, shapes, want, launch, knobs=(), mode=None, together=False, layer=False):
        self.note, self.inputs, self.store, self.shapes, self.want, self.launch = note, inputs, store, shapes, want, launch
        self.knobs, self.mode, self.together, self.layer = knobs, mode, together, layer

    def words(self):
        return Words(self.store, self.shapes, self.together)


def capture_and_replay(hip, plan, case, capture_error_mode="global"):
    import torch
    s = torch.cuda.Stream()
    dev, other = Dev(plan, case.inputs), Dev(plan, case.inputs)
    res, mine = case.words(), case.words()
    torch.cuda.synchronize()

    def replay(times=1):
        with torch.cuda.stream(s):
            for _ in range(times):
                g.replay()

    # 1. one plain call with the same arguments on the capture stream
    held = torch.cuda.memory_allocated()
    assert case.launch(hip, dev, res, s) == 0, (case.note, "plain call", err(hip))
    if case.layer:                             # every result tensor was passed in: the layer allocates nothing
        assert torch.cuda.memory_allocated() == held, (case.note, "the layer allocated", torch.cuda.memory_allocated() - held)
    torch.cuda.synchronize()
    # 2. sentinels
    res.reset()
    # 3. one call captured; the knobs hold around the capture only -- a captured launch no longer looks at them
    g = torch.cuda.CUDAGraph()
    with contextlib.ExitStack() as around:
        for k in case.knobs:
            around.enter_context(k(hip))
        with torch.cuda.graph(g, stream=s, capture_error_mode=capture_error_mode):
            rc = case.launch(hip, dev, res, s)
        assert rc == 0, (case.note, "capturing call", err(hip))
        if case.mode is not None:
            assert case.mode(last_mode(hip)), (case.note, "K1 mode word", last_mode(hip))
    # 4. nothing ran beside the capture
    res.untouched(case.note)
    # 5. three replays; the store form once more over garbage: its zeroing is a node of the graph
    replay(3)
    res.check(case.want["A"], 3, (case.note, "three replays"))
    if case.store:
        res.reset()
        replay()
        res.check(case.want["A"], 1, (case.note, "a replay over garbage"))
    # 6. other contents in the same buffers: a replay counts what is there now
    dev.load("B")
    res.reset()
    replay()
    res.check(case.want["B"], 1, (case.note, "a replay over data set B"))
    # 7. a plain call of the same entry on the capture stream between two replays, on other buffers, into words of its own
    res.reset()
    replay()
    rc = case.launch(hip, other, mine, s)
    replay()
    assert rc == 0, (case.note, "plain call between replays", err(hip))
    res.check(case.want["B"], 2, (case.note, "two replays around a plain call"))
    mine.check(case.want["A"], 1, (case.note, "the plain call between two replays"))


# ------------------------------------------------------------------ K1: the plain, store and superset device entries
K1_ENTRIES = {                                 # name -> (entry, store, superset)
    "u16": ("FLAGSTATS_hip_device_u16", False, False),
    "store": ("FLAGSTATS_hip_device_u16_store", True, False),
    "superset": ("FLAGSTATS_hip_device_u16_superset", False, True),
}
K1_CONFIGS = {                                 # name -> (shape, knob "epilogue", knob "group_max_steps" or None, two-level)
    "edge-direct": ("edge", 1, None, False),
    "edge-k2": ("edge", 0, None, False),
    "grouped-two-level": ("grouped", 1, None, True),
    "grouped-one-level": ("grouped", 1, 0, False),
    "grouped-k2": ("grouped", 0, None, False),
}


def k1_case(plan, entry, config):
    name, store, superset = K1_ENTRIES[entry]
    shape, epilogue, max_steps, two_level = K1_CONFIGS[config]
    n = gp.SHAPES[shape][0]
    knobs = [lambda hip: knob(hip, b"epilogue", epilogue)]
    if max_steps is not None:
        knobs.append(lambda hip: knob(hip, b"group_max_steps", max_steps))

    def mode(m):
        # bit 0 store, bit 1 superset, bit 2 direct (atomic) epilogue, bit 3 its two-level form; the store form always ends in K2
        direct = bool(epilogue) and not store
        return (bool(m & 1), bool(m & 2), bool(m & 4), bool(m & 8)) == (store, superset, direct, direct and two_level)

    def launch(hip, dev, words, stream):
        return getattr(hip, name)(dev.ptr(("flags", shape)), n, words.ptr("out"), raw(stream))

    return Case((entry, config), [("flags", shape)], store, {"out": (32,)}, wants(plan, ("k1", shape), superset), launch, knobs, mode)


@pytest.mark.parametrize("config", list(K1_CONFIGS))
@pytest.mark.parametrize("entry", list(K1_ENTRIES))
def test_k1_entries(hip, plan, entry, config):
    """FLAGSTATS_hip_device_u16, _store and _superset over the edge shape (three workgroups: a head edge step, a fast step, a tail
    edge step) and the grouped shape (101 workgroups), captured in every epilogue form -- K1's direct adds in one level and through
    the workspace's per-XCD copies and tickets (two levels), and K1 + K2 -- with the knob that chose the form set back before the
    first replay.  The two-level form leaves tickets and copies in the stream's workspace for the next replay and for the plain
    launch between two replays."""
    capture_and_replay(hip, plan, k1_case(plan, entry, config))


@pytest.mark.parametrize("shape", list(gp.SHAPES))
def test_pospopcnt_entry(hip, plan, shape):
    """FLAGSTATS_hip_device_pospopcnt_u16 over a periodic array of both shapes: out[16] += bit counts"""
    n = gp.SHAPES[shape][0]

    def launch(hip, dev, words, stream):
        return hip.FLAGSTATS_hip_device_pospopcnt_u16(dev.ptr(("periodic", shape)), n, words.ptr("out"), raw(stream))

    capture_and_replay(hip, plan, Case(("pospopcnt", shape), [("periodic", shape)], False, {"out": (16,)}, wants(plan, ("pospopcnt", shape)), launch))


# ------------------------------------------------------------------ the entries without a workspace
def segments_case(plan, mode):
    def launch(hip, dev, words, stream):
        return hip.FLAGSTATS_hip_device_u16_segments(dev.ptr(FLAGS), N, dev.ptr(OFFSETS), NSEG, words.ptr("out"), mode, raw(stream))

    return Case(("segments", mode), [FLAGS, OFFSETS], bool(mode & STORE), {"out": (NSEG, 32)}, wants(plan, "segments", bool(mode & SUPERSET)),
                launch, knobs=[chain_from_one_unit])


@pytest.mark.parametrize("mode", [STORE, 0, STORE | SUPERSET, SUPERSET])
def test_segments_entry(hip, plan, mode):
    """FLAGSTATS_hip_device_u16_segments: 40 segments (two empty, short ones, one of three units) in the store form -- an
    nseg * 256-byte memset in front of the kernel -- and the += form, plain and superset.  The device offsets are data: data set B
    moves every boundary, and the replay must follow.  Captured under min_units = 1 (the chain runs), replayed under the shipped 2."""
    capture_and_replay(hip, plan, segments_case(plan, mode))


def where_case(plan, encoding, mode):
    sel, sel_offset, sel_bits = (SEL_BITMAP, gp.BIT_OFFSET, 1) if encoding == "bitmap" else (SEL_BYTES, 0, 8)

    def launch(hip, dev, words, stream):
        return hip.FLAGSTATS_hip_device_u16_where(dev.ptr(FLAGS), N, dev.ptr(sel), sel_offset, sel_bits, words.ptr("out"),
                                                  words.ptr("selected"), mode, raw(stream))

    return Case(("where", encoding, mode), [FLAGS, sel], bool(mode & STORE), {"out": (32,), "selected": (1,)},
                wants(plan, "where", bool(mode & SUPERSET)), launch)


@pytest.mark.parametrize("mode", BOTH_MODES)
@pytest.mark.parametrize("encoding", ["bytes", "bitmap"])
def test_where_entry(hip, plan, encoding, mode):
    """FLAGSTATS_hip_device_u16_where under a byte mask and under a bitmap read from bit 5 on (the shifted-bitmap kernel is the
    one captured), store + superset (one memset per pointer) and +="""
    capture_and_replay(hip, plan, where_case(plan, encoding, mode))


def filter_case(plan, with_mapq, mode, together=False):
    key, mn = ("filter_mapq", gp.MIN_MAPQ) if with_mapq else ("filter", 0)

    def launch(hip, dev, words, stream):
        return hip.FLAGSTATS_hip_device_u16_filter(dev.ptr(FLAGS), N, gp.REQUIRE, gp.EXCLUDE, dev.ptr(MAPQ) if with_mapq else None, mn,
                                                   words.ptr("out"), words.ptr("selected"), mode, raw(stream))

    return Case(("filter", key, mode), [FLAGS, MAPQ], bool(mode & STORE), {"out": (32,), "selected": (1,)},
                wants(plan, key, bool(mode & SUPERSET)), launch, together=together)


@pytest.mark.parametrize("mode", BOTH_MODES)
@pytest.mark.parametrize("with_mapq", [False, True])
def test_filter_entry(hip, plan, with_mapq, mode):
    """FLAGSTATS_hip_device_u16_filter without a MAPQ column and with one at byte alignment 3 under threshold 30"""
    capture_and_replay(hip, plan, filter_case(plan, with_mapq, mode))


def segments_filter_case(plan, mode):
    def launch(hip, dev, words, stream):
        return hip.FLAGSTATS_hip_device_u16_segments_filter(dev.ptr(FLAGS), N, dev.ptr(OFFSETS), NSEG, gp.REQUIRE, gp.EXCLUDE, dev.ptr(MAPQ),
                                                            gp.MIN_MAPQ, words.ptr("out"), words.ptr("selected"), mode, raw(stream))

    return Case(("segments_filter", mode), [FLAGS, OFFSETS, MAPQ], bool(mode & STORE), {"out": (NSEG, 32), "selected": (NSEG,)},
                wants(plan, "segments_filter", bool(mode & SUPERSET)), launch, knobs=[chain_from_one_unit])


@pytest.mark.parametrize("mode", BOTH_MODES)
def test_segments_filter_entry(hip, plan, mode):
    """FLAGSTATS_hip_device_u16_segments_filter with the MAPQ column: rows and per-segment counts, the store form's two memsets"""
    capture_and_replay(hip, plan, segments_filter_case(plan, mode))


def wide_case(plan, W, together, mode):
    def launch(hip, dev, words, stream):
        return hip.FLAGSTATS_hip_device_wide(dev.ptr(("wide", W)), N, W, words.ptr("out"), words.ptr("high"), mode, raw(stream))

    return Case(("wide", W, together, mode), [("wide", W)], bool(mode & STORE), {"out": (32,), "high": (1,)},
                wants(plan, ("wide", W), bool(mode & SUPERSET)), launch, together=together)


@pytest.mark.parametrize("mode", BOTH_MODES)
@pytest.mark.parametrize("together", [True, False])
@pytest.mark.parametrize("W", gp.WIDTHS)
def test_wide_entry(hip, plan, W, together, mode):
    """FLAGSTATS_hip_device_wide over int32 and int64 columns with a few elements above bit 15 and one negative one: once with
    d_high == d_out + 32 (the store form's single memset zeroes both), once with separate allocations (one memset each)"""
    capture_and_replay(hip, plan, wide_case(plan, W, together, mode))


def wide_filter_case(plan, W, together, mode):
    def launch(hip, dev, words, stream):
        return hip.FLAGSTATS_hip_device_wide_filter(dev.ptr(("wide", W)), N, W, gp.REQUIRE, gp.EXCLUDE, dev.ptr(MAPQ), gp.MIN_MAPQ,
                                                    words.ptr("out"), words.ptr("selected"), words.ptr("high"), mode, raw(stream))

    return Case(("wide_filter", W, together, mode), [("wide", W), MAPQ], bool(mode & STORE), {"out": (32,), "selected": (1,), "high": (1,)},
                wants(plan, ("wide_filter", W), bool(mode & SUPERSET)), launch, together=together)


@pytest.mark.parametrize("mode", BOTH_MODES)
@pytest.mark.parametrize("together", [True, False])
@pytest.mark.parametrize("W", gp.WIDTHS)
def test_wide_filter_entry(hip, plan, W, together, mode):
    """FLAGSTATS_hip_device_wide_filter: d_out, d_selected and d_high one behind the other (one memset in all) and apart"""
    capture_and_replay(hip, plan, wide_filter_case(plan, W, together, mode))


@pytest.mark.parametrize("which", ["k1", "filter"])
def test_thread_local_capture_mode(hip, plan, which):
    """the same protocol with capture_error_mode="thread_local": K1's two-level form and the filtered store form"""
    case = k1_case(plan, "u16", "grouped-two-level") if which == "k1" else filter_case(plan, True, STORE | SUPERSET)
    capture_and_replay(hip, plan, case, capture_error_mode="thread_local")


# ------------------------------------------------------------------ the torch layers
def _predicate():
    return dict(require=gp.REQUIRE, exclude=gp.EXCLUDE, min_mapq=gp.MIN_MAPQ)


def layer_count(dev, r):
    from libflagstats_amd import device
    return (device.count_torch(dev.view(FLAGS), r.get("out")),)


def layer_pospopcnt(dev, r):
    from libflagstats_amd import device
    return (device.pospopcnt_torch(dev.view(("periodic", "edge")), r.get("out")),)


def layer_segments(dev, r):
    from libflagstats_amd import segments
    return (segments.count_segments_torch(dev.view(FLAGS), dev.view(OFFSETS), out=r.get("out"), store=True, superset=True),)


def layer_where(dev, r):
    import torch
    from libflagstats_amd import where
    return where.count_torch_where(dev.view(FLAGS), dev.view(SEL_BYTES).view(torch.bool), out=r.get("out"), selected=r.get("selected"),
                                   superset=True)


def layer_filter(dev, r):
    from libflagstats_amd import filter as flt
    return flt.count_torch_filter(dev.view(FLAGS), mapq=dev.view(MAPQ), out=r.get("out"), selected=r.get("selected"), store=True,
                                  **_predicate())


def layer_segments_filter(dev, r):
    from libflagstats_amd import segments_filter
    return segments_filter.count_segments_torch_filter(dev.view(FLAGS), dev.view(OFFSETS), mapq=dev.view(MAPQ), out=r.get("out"),
                                                       selected=r.get("selected"), store=False, superset=True, **_predicate())


def layer_ints(dev, r):
    from libflagstats_amd import wide
    return wide.count_torch_ints(dev.view(("wide", 4)), out=r.get("out"), high=r.get("high"))


def layer_ints_filter(dev, r):
    from libflagstats_amd import wide_filter
    return wide_filter.count_torch_ints_filter(dev.view(("wide", 8)), mapq=dev.view(MAPQ), out=r.get("out"), selected=r.get("selected"),
                                               high=r.get("high"), store=True, superset=True, **_predicate())


LAYERS = {    # name -> (call, inputs, result shapes in the order the layer returns them, store, plan key, superset)
    "device.count_torch": (layer_count, [FLAGS], {"out": (32,)}, False, ("k1", "edge"), False),
    "device.pospopcnt_torch": (layer_pospopcnt, [("periodic", "edge")], {"out": (16,)}, False, ("pospopcnt", "edge"), True),
    "segments.count_segments_torch": (layer_segments, [FLAGS, OFFSETS], {"out": (NSEG, 32)}, True, "segments", True),
    "where.count_torch_where": (layer_where, [FLAGS, SEL_BYTES], {"out": (32,), "selected": (1,)}, False, "where", True),
    "filter.count_torch_filter": (layer_filter, [FLAGS, MAPQ], {"out": (32,), "selected": (1,)}, True, "filter_mapq", False),
    "segments_filter.count_segments_torch_filter": (layer_segments_filter, [FLAGS, OFFSETS, MAPQ], {"out": (NSEG, 32), "selected": (NSEG,)},
                                                    False, "segments_filter", True),
    "wide.count_torch_ints": (layer_ints, [("wide", 4)], {"out": (32,), "high": (1,)}, False, ("wide", 4), False),
    "wide_filter.count_torch_ints_filter": (layer_ints_filter, [("wide", 8), MAPQ], {"out": (32,), "selected": (1,), "high": (1,)}, True,
                                            ("wide_filter", 8), True),
}


@pytest.mark.parametrize("layer", list(LAYERS))
def test_torch_layers_with_every_result_passed_in(hip, plan, layer):
    """the count_torch_* layers inside torch.cuda.graph with out, selected and high passed in: they pick up the capturing stream
    (a launch on another stream would run beside the capture, or break it), allocate nothing and synchronise nothing"""
    import torch
    call, inputs, shapes, store, key, superset = LAYERS[layer]

    def launch(hip, dev, words, stream):
        with torch.cuda.stream(stream):
            got = call(dev, words.t)
        assert all(g is words.t[name] for g, name in zip(got, shapes))
        return 0

    capture_and_replay(hip, plan, Case(layer, inputs, store, shapes, wants(plan, key, superset), launch, layer=True))


@pytest.mark.parametrize("layer", list(LAYERS))
def test_torch_layers_allocating_their_results_in_the_capture(hip, plan, layer):
    """the same layers with no result tensor passed in: they make them during the capture, out of the graph's pool, and zero those
    of the += form with a node of the graph -- so the returned tensors hold the values of ONE call after every replay, whatever
    the buffers held at capture time"""
    import torch
    call, inputs, shapes, store, key, superset = LAYERS[layer]
    want = wants(plan, key, superset)
    s = torch.cuda.Stream()
    dev = Dev(plan, inputs)
    with torch.cuda.stream(s):
        call(dev, {})
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="global"):
        got = call(dev, {})
    torch.cuda.synchronize()
    assert len(got) == len(shapes)
    for ds, replays in (("A", 2), ("B", 1), ("A", 3)):
        dev.load(ds)
        with torch.cuda.stream(s):
            for _ in range(replays):
                g.replay()
        torch.cuda.synchronize()
        for t, (name, shape) in zip(got, shapes.items()):
            assert t.dtype == torch.int64 and tuple(t.shape) == shape
            assert np.array_equal(u64(t), want[ds][name].reshape(shape)), (layer, ds, name, u64(t).ravel()[:8], want[ds][name].ravel()[:8])


# ------------------------------------------------------------------ one graph of every entry; one forked graph
def test_one_step_graph(hip, plan):
    """every entry captured one after another into ONE graph on one stream.  The nine += forms add into shared words -- a
    [40][32] block whose row 0 also takes the 32-slot entries' counters and the positional popcount's 16, 40 `selected` words, one
    `high` word; three store forms write words of their own.  Replayed twice: the shared words hold bias + twice the sum of the
    oracle values, every store row its own want."""
    import torch
    inputs = [FLAGS, ("periodic", "edge"), OFFSETS, MAPQ, SEL_BITMAP, ("wide", 4), ("wide", 8)]
    dev = Dev(plan, inputs)
    shared = Words(False, {"out": (NSEG, 32), "selected": (NSEG,), "high": (1,)})
    own = {"store": Words(True, {"out": (32,)}), "segments": Words(True, {"out": (NSEG, 32)}),
           "filter": Words(True, {"out": (32,), "selected": (1,)})}
    out, sel, high = shared.ptr("out"), shared.ptr("selected"), shared.ptr("high")
    flags, mapq, offsets = dev.ptr(FLAGS), dev.ptr(MAPQ), dev.ptr(OFFSETS)
    R, X, Q = gp.REQUIRE, gp.EXCLUDE, gp.MIN_MAPQ

    def step(st):
        return [
            hip.FLAGSTATS_hip_device_u16(flags, N, out, st),
            hip.FLAGSTATS_hip_device_u16_store(flags, N, own["store"].ptr("out"), st),
            hip.FLAGSTATS_hip_device_u16_superset(flags, N, out, st),
            hip.FLAGSTATS_hip_device_pospopcnt_u16(dev.ptr(("periodic", "edge")), N, out, st),
            hip.FLAGSTATS_hip_device_u16_segments(flags, N, offsets, NSEG, out, SUPERSET, st),
            hip.FLAGSTATS_hip_device_u16_segments(flags, N, offsets, NSEG, own["segments"].ptr("out"), STORE, st),
            hip.FLAGSTATS_hip_device_u16_where(flags, N, dev.ptr(SEL_BITMAP), gp.BIT_OFFSET, 1, out, sel, 0, st),
            hip.FLAGSTATS_hip_device_u16_filter(flags, N, R, X, None, 0, out, sel, SUPERSET, st),
            hip.FLAGSTATS_hip_device_u16_filter(flags, N, R, X, mapq, Q, own["filter"].ptr("out"), own["filter"].ptr("selected"), STORE | SUPERSET, st),
            hip.FLAGSTATS_hip_device_u16_segments_filter(flags, N, offsets, NSEG, R, X, mapq, Q, out, sel, 0, st),
            hip.FLAGSTATS_hip_device_wide(dev.ptr(("wide", 4)), N, 4, out, high, 0, st),
            hip.FLAGSTATS_hip_device_wide_filter(dev.ptr(("wide", 8)), N, 8, R, X, mapq, Q, out, sel, high, SUPERSET, st),
        ]

    def expected(ds):
        w = plan.want
        total = {"out": np.zeros((NSEG, 32), dtype=np.uint64), "selected": np.zeros(NSEG, dtype=np.uint64), "high": np.zeros(1, dtype=np.uint64)}
        for key, superset in ((("k1", "edge"), False), (("k1", "edge"), True), ("where", False), ("filter", True), (("wide", 4), False),
                              (("wide_filter", 8), True)):
            total["out"][0] += gp.cut(w[key][ds]["out"], superset)
            total["selected"][0] += w[key][ds].get("selected", np.zeros(1, dtype=np.uint64))[0]
            total["high"] |= w[key][ds].get("high", np.zeros(1, dtype=np.uint64))
        total["out"][0, :16] += w["pospopcnt", "edge"][ds]["out"]
        total["out"] += gp.cut(w["segments"][ds]["out"], True) + gp.cut(w["segments_filter"][ds]["out"], False)
        total["selected"] += w["segments_filter"][ds]["selected"]
        stores = {"store": wants(plan, ("k1", "edge"), False)[ds], "segments": wants(plan, "segments", False)[ds],
                  "filter": wants(plan, "filter_mapq", True)[ds]}
        return total, stores

    s = torch.cuda.Stream()
    assert step(raw(s)) == [0] * 12, err(hip)
    torch.cuda.synchronize()
    shared.reset()
    for words in own.values():
        words.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="global"):
        rcs = step(raw(s))
    assert rcs == [0] * 12, (rcs, err(hip))
    shared.untouched("step graph")
    for words in own.values():
        words.untouched("step graph")
    for ds in gp.DATA_SETS:
        dev.load(ds)
        shared.reset()
        with torch.cuda.stream(s):
            g.replay()
            g.replay()
        total, stores = expected(ds)
        shared.check(total, 2, ("step graph", ds))
        for name, words in own.items():
            words.check(stores[name], 2, ("step graph", ds, name))


def test_one_forked_graph(hip, plan):
    """a capture on stream s forks: a second stream waits on s, K1 += runs on s over the grouped shape and on the second stream over
    the edge shape, both into ONE d_out, and s waits for the second stream before the capture ends -- the contract "launches on
    several streams may share d_out" inside one graph.  The second stream comes from torch's high-priority pool, which nothing else
    in the suite draws from: the library meets it, and makes its workspace, under capture.  No environment variable is set; the
    machine's hardware-queue setting stays as it is."""
    import torch
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream(priority=-1)
    assert s2.cuda_stream != s.cuda_stream
    d1, d2 = Dev(plan, [GROUPED]), Dev(plan, [FLAGS])
    n1 = gp.SHAPES["grouped"][0]
    res = Words(False, {"out": (32,)})
    assert hip.FLAGSTATS_hip_device_u16(d1.ptr(GROUPED), n1, res.ptr("out"), raw(s)) == 0, err(hip)
    torch.cuda.synchronize()
    res.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="global"):
        s2.wait_stream(s)
        rc1 = hip.FLAGSTATS_hip_device_u16(d1.ptr(GROUPED), n1, res.ptr("out"), raw(s))
        rc2 = hip.FLAGSTATS_hip_device_u16(d2.ptr(FLAGS), N, res.ptr("out"), raw(s2))
        s.wait_stream(s2)
    assert (rc1, rc2) == (0, 0), err(hip)
    assert last_mode(hip) & 4
    res.untouched("forked graph")
    for ds in gp.DATA_SETS:
        d1.load(ds)
        d2.load(ds)
        res.reset()
        with torch.cuda.stream(s):
            for _ in range(3):
                g.replay()
        want = {"out": plan.want["hist", "grouped"][ds]["out"] + plan.want["hist", "edge"][ds]["out"]}
        res.check(want, 3, ("forked graph", ds))
