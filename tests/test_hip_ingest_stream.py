"""GPU: the sensor-frame ingest (csrc/gs_ingest.hip) and the frame streamer (gradslam_amd/datasets/streaming.py) on the
cases of tests/ingest_cases.py.  tests/test_ingest_cases_cpu.py holds the references used here to float64.

  * the resize kernels against the oracle, bit for bit: sources with a side of 1 or 2, odd sources, one axis only, integer
    and non-integer ratios, a 1 x 1 target, more than one block; both depth dtypes, normalize on and off;
  * the one-launch native conversion against (raw / div) in float64 cast last, bit for bit: pixel counts on both sides of
    one block and of one sweep of the capped grid for {both, depth only, colour only}, raw frames on the device and in
    pinned host memory, outputs inside larger poisoned buffers whose surroundings must keep their bits;
  * its refusals, by the error alone (a refused call launches nothing, so the poisoned outputs keep their bits);
  * the streamer past the wrap of its ring: in order, repeated, skipping and backwards, a second pass, the validity
    promise of a returned frame, requests outside the sequence, and -- through the bookkeeping, with no timing involved --
    that no event recorded before a non-consecutive request is consulted after it;
  * one SLAM run past the wrap, streamed against resident, bit for bit."""
import numpy as np
import pytest
import torch

from gradslam_amd import _C
from gradslam_amd.datasets.synthetic import make_sequence
from tests import ingest_cases as ic

pytestmark = pytest.mark.gpu

POISON = 0x7FC0DEAD            # a quiet NaN with a recognisable payload
GUARD = 64                     # floats around an output (a multiple of 4: the output stays 16-byte aligned)
Refused = _C.HipExtensionError


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "needs the MI355X"
    from gradslam_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


def u16(a, signed=False):
    """numpy uint16 -> torch uint16 (or the int16 view of the same bits)"""
    t = torch.from_numpy(np.array(a, copy=True, order="C").view(np.int16))
    return t if signed else t.view(torch.uint16)


def u8(a):
    return torch.from_numpy(np.array(a, copy=True, order="C"))


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def same_bits(got, want):
    return got.shape == want.shape and torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


def poisoned(n):
    return torch.full((n,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)


def is_poison(t):
    return bool((t.view(torch.int32) == POISON).all())


def guarded(n):
    """(buffer, out): out = n floats in the middle of a poisoned buffer"""
    buf = poisoned(GUARD + n + GUARD)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    return is_poison(buf[:GUARD]) and is_poison(buf[-GUARD:])


# ------------------------------------------------------------------------------------------------ resize kernels
@pytest.mark.parametrize("case", ic.RESIZE_CASES, ids=ic.resize_name)
def test_resize_kernels_match_oracle(ops, oracle, case):
    (H0, W0), (H, W) = case
    raw_d, raw_c = ic.resize_source(H0, W0)
    for div in ic.RESIZE_SCALE_DIVS:
        want = f32(oracle.ingest_depth(raw_d, H, W, div))
        for signed in (False, True):
            got = ops.ingest_depth(u16(raw_d, signed).cuda(), H, W, div)
            assert got.dtype == torch.float32 and same_bits(got, want), (div, signed)
    for normalize in (False, True):
        want = f32(oracle.ingest_color(raw_c, H, W, normalize))
        got = ops.ingest_color(u8(raw_c).cuda(), H, W, normalize)
        assert got.dtype == torch.float32 and same_bits(got, want), normalize


# ------------------------------------------------------------------------------------------------ native conversion
def run_native(ops, shape, d_raw, c_raw, want_d, want_c, tag):
    """every modality mix, normalize setting and scale_div on one pair of raw tensors"""
    n, H, W = shape
    px = n * H * W
    for mode in ic.NATIVE_MODES:
        for normalize in (False, True):
            for div in ic.NATIVE_SCALE_DIVS:
                dbuf, dout = guarded(px)
                cbuf, cout = guarded(3 * px)
                ops.ingest_frames_native(d_raw if mode != "color" else None, c_raw if mode != "depth" else None,
                                         dout if mode != "color" else None, cout if mode != "depth" else None, div, normalize)
                what = (tag, mode, normalize, div)
                if mode != "color":
                    assert same_bits(dout, want_d[div].reshape(-1)), what
                else:
                    assert is_poison(dout), what
                if mode != "depth":
                    assert same_bits(cout, want_c[normalize].reshape(-1)), what
                else:
                    assert is_poison(cout), what
                assert guards_intact(dbuf) and guards_intact(cbuf), what


def native_refs(shape):
    d, c = ic.native_raw(shape)
    return ({div: f32(ic.native_depth_ref(d, div)) for div in ic.NATIVE_SCALE_DIVS},
            {norm: f32(ic.native_color_ref(c, norm)) for norm in (False, True)})


@pytest.mark.parametrize("shape", ic.NATIVE_SHAPES, ids=ic.native_name)
def test_native_conversion_matches_float64_device_frames(ops, shape):
    d, c = ic.native_raw(shape)
    want_d, want_c = native_refs(shape)
    for signed in (False, True):       # the int16 view of depths at or above 32768 reads as unsigned
        run_native(ops, shape, u16(d, signed).cuda(), u8(c).cuda(), want_d, want_c, "int16" if signed else "uint16")


@pytest.mark.parametrize("shape", [min(ic.NATIVE_SHAPES, key=lambda s: s[0] * s[1] * s[2]),
                                   max(ic.NATIVE_SHAPES, key=lambda s: s[0] * s[1] * s[2])], ids=ic.native_name)
def test_native_conversion_matches_float64_pinned_host_frames(ops, shape):
    d, c = ic.native_raw(shape)
    want_d, want_c = native_refs(shape)
    d_host, c_host = u16(d).pin_memory(), u8(c).pin_memory()
    assert ops.host_device_pointer(d_host) is not None and ops.host_device_pointer(c_host) is not None
    run_native(ops, shape, d_host, c_host, want_d, want_c, "pinned")


# ------------------------------------------------------------------------------------------------ refusals
def test_native_conversion_refuses_what_it_cannot_convert(ops):
    n, H, W = 2, 4, 6
    px = n * H * W
    d = u16(np.zeros((n, H, W), np.uint16)).cuda()
    c = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    d_wide = u16(np.zeros(px + 8, np.uint16)).cuda()
    c_wide = torch.zeros(3 * px + 8, dtype=torch.uint8, device="cuda")
    dbuf, cbuf = poisoned(px + 8), poisoned(3 * px + 8)
    dout, cout = dbuf[:px], cbuf[:3 * px]
    assert d_wide.data_ptr() % 8 == 0 and c_wide.data_ptr() % 4 == 0 and dbuf.data_ptr() % 16 == 0 and cbuf.data_ptr() % 16 == 0
    d_off, c_off = d_wide[1:1 + px].view(n, H, W), c_wide[1:1 + 3 * px].view(n, H, W, 3)
    assert d_off.data_ptr() % 8 == 2 and c_off.data_ptr() % 4 == 1 and d_off.is_contiguous() and c_off.is_contiguous()
    d15 = u16(np.zeros((1, 3, 5), np.uint16)).cuda()
    c15 = torch.zeros((1, 3, 5, 3), dtype=torch.uint8, device="cuda")
    refused = [
        ("px % 4", (d15, c15, dbuf[:15], cbuf[:45]), "multiple of 4"),
        ("px % 4, depth only", (d15, None, dbuf[:15], None), "multiple of 4"),
        ("px % 4, colour only", (None, c15, None, cbuf[:45]), "multiple of 4"),
        ("raw depth one element in", (d_off, c, dout, cout), "misaligned"),
        ("raw depth one element in, depth only", (d_off, None, dout, None), "misaligned"),
        ("raw colour one byte in", (d, c_off, dout, cout), "misaligned"),
        ("raw colour one byte in, colour only", (None, c_off, None, cout), "misaligned"),
        ("depth out one float in", (d, c, dbuf[1:1 + px], cout), "misaligned"),
        ("colour out one float in", (d, c, dout, cbuf[1:1 + 3 * px]), "misaligned"),
        ("depth out too large", (d, c, dbuf[:px + 4], cout), "do not match"),
        ("colour out too small", (d, c, dout, cbuf[:3 * px - 12]), "do not match"),
        ("colour of another pixel count", (d, c[:1], dout, cbuf[:3 * px // 2]), "do not match"),
        ("float32 raw depth", (torch.zeros((n, H, W), device="cuda"), c, dout, cout), "do not match"),
        ("int8 raw colour", (d, c.view(torch.int8), dout, cout), "do not match"),
        ("float64 out", (d, c, torch.zeros(px, dtype=torch.float64, device="cuda"), cout), "do not match"),
        ("transposed raw depth", (d.transpose(1, 2), c, dout, cout), "do not match"),
        ("strided raw colour", (d, torch.zeros((n, H, W, 6), dtype=torch.uint8, device="cuda")[..., ::2], dout, cout), "do not match"),
        ("host depth, not pinned", (u16(np.zeros((n, H, W), np.uint16)), c, dout, cout), "pinned"),
        ("host colour, not pinned", (d, torch.zeros((n, H, W, 3), dtype=torch.uint8), dout, cout), "pinned"),
        ("depth raw without out", (d, c, None, cout), "in pairs"),
        ("colour raw without out", (d, c, dout, None), "in pairs"),
        ("depth out without raw", (None, c, dout, cout), "in pairs"),
        ("nothing to convert", (None, None, None, None), "in pairs"),
    ]
    for what, (dr, cr, do, co), message in refused:
        with pytest.raises(Refused, match=message):
            ops.ingest_frames_native(dr, cr, do, co, 5000.0)
    torch.cuda.synchronize()
    assert is_poison(dbuf) and is_poison(cbuf), "a refused call wrote to its outputs"
    # and the same buffers are accepted once nothing is wrong with them
    ops.ingest_frames_native(d, c, dout, cout, 5000.0)
    assert bool((dout == 0).all()) and bool((cout == 0).all()) and is_poison(dbuf[px:]) and is_poison(cbuf[3 * px:])


# ------------------------------------------------------------------------------------------------ streamer
SB, SH, SW = 2, 6, 10


def _ring():
    from gradslam_amd.datasets.streaming import FrameStreamer
    return FrameStreamer.RING


@pytest.fixture(scope="module")
def stream_data(ops):
    """pinned raw frames (L = 2 RING + 5), and the resident per-frame conversion of every (t, b): the reference"""
    L = 2 * _ring() + 5
    d, c = ic.stream_content(L, SB, SH, SW)
    d16, c8 = u16(d).pin_memory(), u8(c).pin_memory()
    dres = torch.stack([torch.stack([ops.ingest_depth(d16[t, b].cuda(), SH, SW, 5000.0) for b in range(SB)]) for t in range(L)])
    cres = {norm: torch.stack([torch.stack([ops.ingest_color(c8[t, b].cuda(), SH, SW, norm) for b in range(SB)])
                               for t in range(L)]) for norm in (False, True)}
    # the per-frame kernels at the native size are the float64 statement (the same reference as above)
    assert same_bits(dres, f32(ic.native_depth_ref(d, 5000.0)))
    for norm in (False, True):
        assert same_bits(cres[norm], f32(ic.native_color_ref(c, norm)))
    eye = torch.eye(4, device="cuda").expand(SB, 1, 4, 4).contiguous()
    return {"L": L, "d16": d16, "c8": c8, "dres": dres, "cres": cres, "K": eye, "P0": eye.clone()}


def make_streamer(sd, zero_copy, normalize):
    from gradslam_amd.datasets.streaming import FrameStreamer
    st = FrameStreamer(sd["d16"], sd["c8"], sd["K"], sd["P0"], scale_div=5000.0, device="cuda", normalize_color=normalize,
                       zero_copy=zero_copy)
    assert st.zero_copy == zero_copy and len(st) == sd["L"]
    return st


def holds(sd, frame, t, normalize):
    """the RGBDImages `frame` holds frame t of every sequence, bit for bit"""
    d, c = frame.depth_image, frame.rgb_image
    assert tuple(d.shape) == (SB, 1, SH, SW, 1) and tuple(c.shape) == (SB, 1, SH, SW, 3)
    return same_bits(d[:, 0, ..., 0], sd["dres"][t]) and same_bits(c[:, 0], sd["cres"][normalize][t])


def check_slots(st):
    """every ring slot that claims a frame holds it (the transfers are waited for first)"""
    st.copy_stream.synchronize()
    for k, t in enumerate(st.in_slot):
        assert t == -1 or (0 <= t < st.L and t % st.RING == k), st.in_slot


MODES = [(False, False), (False, True), (True, False), (True, True)]
MODE_IDS = ["copy", "copy-normalized", "zero_copy", "zero_copy-normalized"]


@pytest.mark.parametrize("zero_copy,normalize", MODES, ids=MODE_IDS)
def test_streamer_in_order_reuses_every_slot_and_runs_a_second_pass(stream_data, zero_copy, normalize):
    sd, L = stream_data, stream_data["L"]
    st = make_streamer(sd, zero_copy, normalize)
    R = st.RING
    for rnd in range(2):
        for t in range(L):
            assert holds(sd, st.frame(t), t, normalize), (rnd, t)
            assert st.in_slot[t % R] == t and (t + 1 >= L or st.in_slot[(t + 1) % R] == t + 1)
            assert len(st.done) <= 2 * R + 1
        check_slots(st)
        assert st.in_slot == [max(t for t in range(L) if t % R == k) for k in range(R)]
    st.close()


@pytest.mark.parametrize("zero_copy,normalize", MODES, ids=MODE_IDS)
def test_streamer_serves_repeated_skipping_and_backward_requests(stream_data, zero_copy, normalize):
    sd, L = stream_data, stream_data["L"]
    st = make_streamer(sd, zero_copy, normalize)
    a = st.frame(7)
    assert holds(sd, a, 7, normalize)
    slots = list(st.in_slot)
    b = st.frame(7)
    assert holds(sd, b, 7, normalize) and holds(sd, a, 7, normalize) and st.in_slot == slots
    assert b.depth_image.data_ptr() == a.depth_image.data_ptr()
    for t in (0, 1, 5, 6, 17, 3, 3, L - 1, 0, L - 1, L - 2, 12, 2, 13):
        assert holds(sd, st.frame(t), t, normalize), t
        assert st.in_slot[t % st.RING] == t
    check_slots(st)
    st.close()


@pytest.mark.parametrize("zero_copy", [False, True], ids=["copy", "zero_copy"])
def test_streamer_keeps_a_returned_frame_valid(stream_data, zero_copy):
    """the promise of frame(): the tensors of frame t still hold it after frames up to t + RING - 3 were asked for"""
    sd, L = stream_data, stream_data["L"]
    st = make_streamer(sd, zero_copy, False)
    R = st.RING
    t = 0
    while t + R - 3 < L:
        held = st.frame(t)
        assert holds(sd, held, t, False)
        for u in range(t + 1, t + R - 2):
            assert holds(sd, st.frame(u), u, False), (t, u)
            torch.cuda.synchronize()
            assert holds(sd, held, t, False), (t, u)
        t += R - 2
    assert t > R        # (slots were reused while frames were held)
    st.close()


def ring_bits(st):
    torch.cuda.synchronize()
    return [x.clone() for x in st.f_d + st.f_c]


@pytest.mark.parametrize("zero_copy", [False, True], ids=["copy", "zero_copy"])
def test_streamer_refuses_frames_outside_the_sequence(stream_data, zero_copy):
    sd, L = stream_data, stream_data["L"]
    st = make_streamer(sd, zero_copy, False)
    for before in (0, 3, L - 1):      # on a fresh streamer (slots still empty), in the middle, at the end
        if before:
            for t in range(before - 2, before + 1):
                assert holds(sd, st.frame(t), t, False)
        slots, done, last, bits = list(st.in_slot), dict(st.done), st.last, ring_bits(st)
        for bad in (L, -1, L + st.RING, -st.RING, 10 * L):
            with pytest.raises(IndexError):
                st.frame(bad)
        assert st.in_slot == slots and st.last == last
        assert st.done.keys() == done.keys() and all(st.done[k] is done[k] for k in done)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(ring_bits(st), bits))
    assert holds(sd, st.frame(L - 1), L - 1, False)
    st.close()


def test_streamer_refuses_a_batch_that_is_no_multiple_of_four_pixels(ops):
    from gradslam_amd.datasets.streaming import FrameStreamer
    d, c = ic.stream_content(3, 1, 3, 5)
    eye = torch.eye(4, device="cuda").expand(1, 1, 4, 4).contiguous()
    for zero_copy in (False, True):
        with pytest.raises(Refused, match="the pixel count must be a multiple of 4"):
            FrameStreamer(u16(d).pin_memory(), u8(c).pin_memory(), eye, eye.clone(), 5000.0, zero_copy=zero_copy)


@pytest.mark.parametrize("zero_copy", [False, True], ids=["copy", "zero_copy"])
def test_no_event_survives_a_non_consecutive_request(stream_data, zero_copy):
    """_prefetch looks events up by frame number.  An event recorded in one run of consecutive requests says nothing
    about another run: after a rewind, a skip or a repeat, `done` must hold none of the events it held before (compared
    by identity; the old events are kept alive here, so no new event can take the identity of an old one)."""
    sd, L = stream_data, stream_data["L"]
    st = make_streamer(sd, zero_copy, False)
    R = st.RING
    for t in range(L):
        before = st.done.get(t - 1)
        st.frame(t)
        if t > 0:     # the consecutive path: one new event per frame, under the key of the frame before
            assert st.done[t - 1] is not before and set(st.done) == set(range(max(0, t - 2 * R), t))
    old = list(st.done.values())
    assert len(old) >= R

    def none_of_the_old():
        return not any(ev is o for ev in st.done.values() for o in old)

    assert holds(sd, st.frame(0), 0, False)           # the rewind
    assert none_of_the_old() and not st.done
    for t in range(1, L):                              # the whole second pass
        assert holds(sd, st.frame(t), t, False), t
        assert none_of_the_old() and set(st.done) <= set(range(0, t)), t
    for t in (5, 6, 7, 7, 8, 20, 21, 2):               # a rewind into the middle, a repeat, a skip, a rewind
        consecutive = t == st.last + 1
        if not consecutive:
            old += list(st.done.values())
        assert holds(sd, st.frame(t), t, False), t
        assert none_of_the_old(), t
        assert (t - 1 in st.done) == consecutive and len(st.done) <= (3 if consecutive else 0), (t, sorted(st.done))
    st.close()


# ------------------------------------------------------------------------------------------------ through the SLAM step
def test_slam_run_past_the_wrap_streamed_equals_resident(ops):
    import gradslam_amd as gs
    from gradslam_amd.datasets.streaming import FrameStreamer, quantize_sequences
    B, H, W = 2, 60, 80
    L = FrameStreamer.RING + 3
    seqs = [make_sequence(L, H, W, seed=71 + b) for b in range(B)]
    d16, c8 = quantize_sequences(seqs, 5000.0)
    dres = torch.stack([torch.stack([ops.ingest_depth(d16[t, b].cuda(), H, W, 5000.0) for t in range(L)]) for b in range(B)])
    cres = torch.stack([torch.stack([ops.ingest_color(c8[t, b].cuda(), H, W) for t in range(L)]) for b in range(B)])
    K = torch.from_numpy(np.stack([s["intrinsics"] for s in seqs])).cuda()
    P0 = torch.from_numpy(np.stack([s["poses"][:1] for s in seqs])).cuda()
    frames = gs.RGBDImages(cres, dres[..., None], K, P0.repeat(1, L, 1, 1))

    def run(get):
        slam = gs.slam.PointFusion(odom="gradicp", device="cuda")
        pc, prev, rec = gs.Pointclouds(device="cuda"), None, []
        for t in range(L):
            live = get(t)
            pc, p = slam.step(pc, live, prev, inplace=True)
            prev = live
            rec.append(p[:, 0].cpu().numpy())
        return np.stack(rec), [x.cpu().numpy() for x in pc.points_list], [x.cpu().numpy() for x in pc.colors_list]

    ref = run(lambda t: frames[:, t])
    assert np.isfinite(ref[0]).all() and all(len(x) > 0 for x in ref[1])
    for zero_copy in (False, True):
        st = FrameStreamer(d16, c8, K, P0, scale_div=5000.0, device="cuda", zero_copy=zero_copy)
        assert st.zero_copy == zero_copy
        got = run(st.frame)
        assert max(st.in_slot) == L - 1 and sorted(st.in_slot)[0] >= L - st.RING       # the ring wrapped
        assert np.array_equal(ref[0].view(np.int32), got[0].view(np.int32))
        for a, b in zip(ref[1] + ref[2], got[1] + got[2]):
            assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
        st.close()
