"""orient_brief_kernel (orbx_brief.hip) over batch sizes, sparse frames and small
levels, against the oracle bit for bit.

Written for a kernel whose waves take a contiguous run of a frame's keypoint
pairs (slots 2p, 2p + 1) instead of one pair each: a frame gets `wgs`
workgroups of 4 waves, wave q of the 4 * wgs takes pairs / (4 * wgs) pairs and
the first pairs % (4 * wgs) waves one more; a launch the chip holds at once
keeps one pair per wave, larger ones loop, step over a level's padding slots,
change level inside a run and store a pair's results during the next pair's
turn. That kernel was measured and not kept ("orient+BRIEF: sincosf
tables in LDS; long-lived waves measured and rejected"); the kernel in the tree
takes one pair per wave at every batch size, and these cases hold for any
mapping of slots to waves. The batch sizes come from a mirror of that
kernel's launch rule (_wgs), so that a kernel which takes the rule up again
meets its run lengths here: 1, 2, uneven, 3 and more, 8 and more.
"""
import functools

import numpy as np
import pytest

from test_gpu_extract import assert_same, oracle_cfg

pytestmark = pytest.mark.gpu

CUS = 256       # MI355X
WG_PER_CU = 6   # resident workgroups per CU (26 KB of LDS each)
FILL = 1        # the rule's factor on the resident workgroups
KPS = 8         # kObKps = kKpGroup (orbx_brief.hip, orbx_internal.h): slots per group
FILL_BYTE = 0xA5


def _wgs(B, groups):
    """Workgroups per frame of a launch of B frames: one per group of 8 slots while
    the chip holds groups * B workgroups at once, else FILL x the resident ones."""
    resident = CUS * WG_PER_CU
    if groups * B <= resident:
        return groups
    return min(max(-(-resident * FILL // B), 1), groups)


def _runs(B, groups):
    """(run, rem): every wave of a frame takes `run` pairs, the first `rem` one more."""
    pairs, waves = groups * KPS // 2, 4 * _wgs(B, groups)
    return pairs // waves, pairs % waves


def _smallest_batch(groups, pred, limit=2048):
    for B in range(1, limit + 1):
        if pred(*_runs(B, groups)):
            return B
    raise AssertionError("no batch size up to %d gives the wanted runs" % limit)


def _looping_batch(groups):
    """The smallest batch whose waves all take two pairs or more."""
    return _smallest_batch(groups, lambda run, rem: run >= 2)


@functools.lru_cache(maxsize=None)
def _frames(seed, W, H):
    from orb_slam_cuda_amd.synth import synth_frame
    return tuple(synth_frame(seed + i, W, H) for i in range(3))


_REFS = {}


def _ref(O, key, cfg, img):
    """The oracle's extraction of a frame, computed once per module run."""
    if key not in _REFS:
        _REFS[key] = O.extract(cfg, img)
    return _REFS[key]


def _run(pkg, ext, frames, order):
    """One extract_batch_device launch of frames[order[b]]; outputs prefilled with FILL_BYTE.
    Returns (counts, keypoint records as bytes [B, cap, 28], descriptors [B, cap, 32])."""
    from orb_slam_cuda_amd import _lib
    B, (H, W), cap = len(order), frames[0].shape, ext.frame_capacity
    host = np.stack([frames[i] for i in order])
    d_in = _lib.DeviceArray(host.nbytes)
    d_in.upload(host)
    d_kp, d_desc, d_n = _lib.DeviceArray(B * cap * 28), _lib.DeviceArray(B * cap * 32), _lib.DeviceArray(B * 4)
    d_kp.upload(np.full(B * cap * 28, FILL_BYTE, np.uint8))
    d_desc.upload(np.full(B * cap * 32, FILL_BYTE, np.uint8))
    d_n.upload(np.full(B * 4, FILL_BYTE, np.uint8))
    s = _lib.Stream()
    ext.extract_batch_device(d_in.ptr, B, H * W, W, d_kp.ptr, d_desc.ptr, d_n.ptr, s)
    s.synchronize()
    return (d_n.download(B, np.int32), d_kp.download((B, cap, 28), np.uint8),
            d_desc.download((B, cap, 32), np.uint8))


def _check_frame(pkg, out, b, rkp, rdesc):
    """Frame b of a launch equals the oracle's (rkp, rdesc), and nothing was
    written at or beyond its count."""
    n, kps, descs = out
    assert n[b] == len(rkp), (b, n[b], len(rkp))
    assert_same(kps[b, :n[b]].copy().view(pkg.KP_DTYPE).reshape(-1), descs[b, :n[b]], rkp, rdesc)
    assert (kps[b, n[b]:] == FILL_BYTE).all(), ("keypoints written beyond the count", b)
    assert (descs[b, n[b]:] == FILL_BYTE).all(), ("descriptors written beyond the count", b)


def _groups(ext):
    assert ext.frame_capacity % KPS == 0
    return ext.frame_capacity // KPS


# ---------------------------------------------------------------- loop lengths
EUROC = dict(nf=1000, W=752, H=480)

LOOPS = {
    "one_pair": lambda run, rem: (run, rem) == (1, 0),
    "two_pairs": lambda run, rem: run + (rem > 0) >= 2,    # the smallest batch at which a wave takes 2
    "uneven": lambda run, rem: run >= 2 and rem > 0,       # some waves k pairs, some k - 1
    "three_up": lambda run, rem: run >= 3,
}


@pytest.mark.parametrize("kind", list(LOOPS))
def test_loop_lengths(pkg, O, kind):
    """752 x 480, 1000 features, 8 levels, three frames repeated: one pair per
    wave, the first batch with two, uneven runs and runs of three or more."""
    nf, W, H = EUROC["nf"], EUROC["W"], EUROC["H"]
    frames = _frames(100, W, H)
    cfg = oracle_cfg(O, nf, W, H)
    groups = _groups(pkg.ORBextractor(nf, 1.2, 8, 20, 7, W, H))
    B = _smallest_batch(groups, LOOPS[kind])
    if kind == "one_pair":
        assert B == 1
    ext = pkg.ORBextractor(nf, 1.2, 8, 20, 7, W, H, max_batch=B)
    out = _run(pkg, ext, frames, [b % 3 for b in range(B)])
    for b in sorted({0, min(1, B - 1), min(2, B - 1), B - 1}):
        _check_frame(pkg, out, b, *_ref(O, ("euroc", b % 3), cfg, frames[b % 3]))


# ---------------------------------------------------------------- sparse frames
def _sparse_frames(W, H):
    from orb_slam_cuda_amd.synth import synth_frame
    normal = synth_frame(41, W, H)
    corner = np.full((H, W), 128, np.uint8)
    corner[:64, :64] = normal[:64, :64]
    return np.zeros((H, W), np.uint8), corner, normal


@pytest.mark.parametrize("black_at_ends", [False, True])
def test_sparse_frames(pkg, O, black_at_ends):
    """A black frame (count 0, still written), a frame textured in one 64 x 64
    corner only (levels with odd and tiny counts: half-valid pairs, pairs
    stepped over) and a normal frame in one looping batch; then with the black
    frame first and last."""
    nf, W, H = 600, 640, 240
    frames = _sparse_frames(W, H)
    cfg = oracle_cfg(O, nf, W, H)
    refs = [_ref(O, ("sparse", i), cfg, frames[i]) for i in range(3)]
    assert len(refs[0][0]) == 0 and 0 < len(refs[1][0]) < len(refs[2][0])
    groups = _groups(pkg.ORBextractor(nf, 1.2, 8, 20, 7, W, H))
    B = max(_looping_batch(groups), 6)
    order = [(b + 1) % 3 for b in range(B)]
    if black_at_ends:
        order = [0] + [1 + b % 2 for b in range(B - 2)] + [0]
    ext = pkg.ORBextractor(nf, 1.2, 8, 20, 7, W, H, max_batch=B)
    out = _run(pkg, ext, frames, order)
    assert out[0][0] == (0 if black_at_ends else len(refs[1][0]))
    for b in range(B):
        _check_frame(pkg, out, b, *refs[order[b]])


# ------------------------------------------------- level switches inside a run
@pytest.mark.parametrize("looping", [False, True])
def test_level_switches_inside_a_run(pkg, O, looping):
    """100 features over 8 levels of 320 x 240: level slot ranges of 8 to 24
    slots, so a run of 8 pairs or more crosses several levels."""
    nf, W, H = 100, 320, 240
    frames = _frames(7, W, H)
    cfg = oracle_cfg(O, nf, W, H)
    groups = _groups(pkg.ORBextractor(nf, 1.2, 8, 20, 7, W, H))
    assert groups * KPS <= 8 * 24
    B = _smallest_batch(groups, lambda run, rem: run >= 8) if looping else 1
    ext = pkg.ORBextractor(nf, 1.2, 8, 20, 7, W, H, max_batch=B)
    out = _run(pkg, ext, frames, [b % 3 for b in range(B)])
    for b in sorted({0, min(1, B - 1), min(2, B - 1), B - 1}):
        _check_frame(pkg, out, b, *_ref(O, ("small", b % 3), cfg, frames[b % 3]))


# --------------------------------------------------------------------- variants
def test_ten_levels(pkg, O):
    """10 levels (1226 x 370, thresholds 17 / 7, 2000 features): the kernel's
    kMaxLevels instantiation, at B = 2 and in a looping batch."""
    nf, W, H = 2000, 1226, 370
    frames = _frames(55, W, H)
    cfg = oracle_cfg(O, nf, W, H, nlevels=10, ini=17, mn=7)
    groups = _groups(pkg.ORBextractor(nf, 1.2, 10, 17, 7, W, H))
    for B in (2, _looping_batch(groups)):
        ext = pkg.ORBextractor(nf, 1.2, 10, 17, 7, W, H, max_batch=B)
        out = _run(pkg, ext, frames, [b % 3 for b in range(B)])
        for b in sorted({0, 1, min(2, B - 1), B - 1}):
            _check_frame(pkg, out, b, *_ref(O, ("ten", b % 3), cfg, frames[b % 3]))


def test_upstream_pattern(pkg, O):
    """The upstream BRIEF table in a looping batch."""
    nf, W, H = EUROC["nf"], EUROC["W"], EUROC["H"]
    frames = _frames(100, W, H)
    cfg = oracle_cfg(O, nf, W, H, pattern="upstream")
    groups = _groups(pkg.ORBextractor(nf, 1.2, 8, 20, 7, W, H, pattern="upstream"))
    B = _looping_batch(groups)
    ext = pkg.ORBextractor(nf, 1.2, 8, 20, 7, W, H, max_batch=B, pattern="upstream")
    out = _run(pkg, ext, frames, [b % 3 for b in range(B)])
    for b in sorted({0, 1, 2, B - 1}):
        _check_frame(pkg, out, b, *_ref(O, ("upstream", b % 3), cfg, frames[b % 3]))


# ------------------------------------------------------------------ determinism
def test_same_launch_twice(pkg):
    """The same looping launch twice: identical counts, keypoint and descriptor bytes."""
    nf, W, H = EUROC["nf"], EUROC["W"], EUROC["H"]
    frames = _frames(100, W, H)
    groups = _groups(pkg.ORBextractor(nf, 1.2, 8, 20, 7, W, H))
    B = _smallest_batch(groups, LOOPS["uneven"])
    ext = pkg.ORBextractor(nf, 1.2, 8, 20, 7, W, H, max_batch=B)
    order = [b % 3 for b in range(B)]
    first, second = _run(pkg, ext, frames, order), _run(pkg, ext, frames, order)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
