"""The extractor's host plan (csrc/orbx_plan.hip), checked without a GPU.

The plan is what turns a configuration into kernel parameters and tables: a
wrong entry is an out-of-bounds access on the device. orbx_plan_digest plans a
configuration on the host and returns FNV-1a digests of the parameter block
(field by field, no padding byte), the FAST cell table and the resize table
(resize coefficients, the band pyramid's records, quadtree code tables, blur
work lists). They are compared with the digests of the plan the library made
before orbx_host.hip was split (RECORDED below), bit for bit.
"""
import ctypes as C

import pytest

import orb_slam_cuda_amd as pkg
from test_gpu_pyramid_direct import GEOMETRIES

KITTI = ("kitti", 1241, 376, 8, 1.2, 64)
# GEOMETRIES has 16 entries; five more of other shapes: one-frame plans, an odd size at
# another scale factor, 12 levels, a 2048-wide frame
MORE = [("tum", 640, 480, 8, 1.2, 1), ("hd", 1280, 720, 8, 1.2, 8), ("kitti_b1", 1241, 376, 8, 1.2, 1),
        ("odd", 1023, 767, 6, 1.3, 2), ("deep", 2048, 1536, 12, 1.2, 1)]
# (case, scale_mode, environment)
CASES = [(g, 0, {}) for g in GEOMETRIES + MORE] + \
        [(("kitti_modeF", 1241, 376, 8, 1.2, 64), 1, {}),
         (KITTI, 0, {"ORBX_QT_GENERIC": "1"}), (KITTI, 0, {"ORBX_QT_SORTED": "0"})]


def _key(case, mode, env):
    switches = " ".join("%s=%s" % kv for kv in sorted(env.items()))
    return ("%s %dx%d L%d sf%g B%d mode%d %s" % (case + (mode, switches))).strip()


# Recorded from commit 5c4e9ce (the parent of the split), with the same digest
# function: the block "plan digest" of csrc/orbx_plan.hip appended to that
# commit's csrc/orbx_host.hip in a scratch worktree (tools/build_parent_lib.sh
# shows how to make one) with an orbx_plan_digest that calls compute_scales,
# build_plan_host and plan_digest on a fresh orbx_extractor; the library built
# with make and these cases run through _digest() below. The patch is not kept.
RECORDED = {
    "kitti 1241x376 L8 sf1.2 B64 mode0": (0x3096c53ecf3bbba7, 0x145ea9f0f3b41a9e, 0x57d5ce2a9505c21b),
    "euroc 752x480 L8 sf1.2 B64 mode0": (0xde42189b24c8e54b, 0xd844a3c5b42e8707, 0x091a2a219e054913),
    "kitti14 1226x370 L10 sf1.2 B64 mode0": (0xf0a050174774d117, 0x56d3173b5ff56c5f, 0x8544dcf0da9386ad),
    "intcatch1080 1920x1080 L3 sf1.2 B16 mode0": (0x358319e44a5207d9, 0xcd2acc1038b7b823, 0xf1840837fa65b5a1),
    "small 208x131 L4 sf1.2 B3 mode0": (0xa680e4f3203cb3ac, 0x64a21e0efbbc9048, 0x80d64e3bcc6a54d8),
    "small 209x131 L4 sf1.2 B3 mode0": (0x8f2589d0d2011ad9, 0x585e8e0839e238b8, 0x77bc1c1162823dcd),
    "small 201x131 L4 sf1.2 B3 mode0": (0x92c4428aab4eafab, 0x7e028b5aeda5e0f7, 0xd3c4a819d2801fa1),
    "small 203x131 L4 sf1.2 B3 mode0": (0x87189e7d510702c5, 0x004fa8b3effa9490, 0xdfa469003c892903),
    "small 207x131 L4 sf1.2 B3 mode0": (0xc8ba9eab232dba4b, 0x3ee4dbe852ec0c13, 0x57ed1adc4ddd6d9b),
    "small 219x140 L4 sf1.2 B3 mode0": (0x040d174471411470, 0x1cbd6e6f6c1778c6, 0x88801be47ad0a149),
    "small 640x131 L4 sf1.2 B3 mode0": (0x153a15019095ceca, 0x2b20ed93695d09e9, 0xdc013f1eff09e81e),
    "small2 203x131 L2 sf2 B3 mode0": (0xc1b9048bd8f69e64, 0xd3b2efb69a939ec2, 0xebb846bc6d89abc4),
    "small2 204x132 L2 sf2 B3 mode0": (0x4ba8be95104bd8bb, 0xaf117afd589aaef6, 0xd5afa2567ce96087),
    "l8 651x459 L8 sf1.2 B3 mode0": (0xe8432ce2b8f5cf50, 0xedd6995e1c067299, 0x07437edc41caaa0a),
    "s2 652x520 L3 sf2 B3 mode0": (0x2521d671cc91e961, 0xda44514783cf00f0, 0x97605d7e0ecefe8a),
    "s2 651x519 L3 sf2 B3 mode0": (0xed1e524074e0efd9, 0x310563f2e85b3962, 0xb967d9e61e38fceb),
    "tum 640x480 L8 sf1.2 B1 mode0": (0xc3cdaff2f334f648, 0x8a039ea29fc10328, 0xffdc078f8b69df3a),
    "hd 1280x720 L8 sf1.2 B8 mode0": (0x1a0f0d1310ae817d, 0xdc3da35564411113, 0x57a77456cfe8753a),
    "kitti_b1 1241x376 L8 sf1.2 B1 mode0": (0x8bdc20bfb1153bc9, 0x884708db8b04352e, 0x57d5ce2a9505c21b),
    "odd 1023x767 L6 sf1.3 B2 mode0": (0xdc9917ca692cc9e8, 0x194f8ae32fe1a745, 0x5ba828c14412a13c),
    "deep 2048x1536 L12 sf1.2 B1 mode0": (0x31bfe8e50c7edfb6, 0x905841b075b16c30, 0xe933755ad98987dd),
    "kitti_modeF 1241x376 L8 sf1.2 B64 mode1": (0x43208799d448205d, 0x610ec84ccf8902ef, 0x7a4e3018634ca468),
    "kitti 1241x376 L8 sf1.2 B64 mode0 ORBX_QT_GENERIC=1": (0x4b0d5895fadd3e2a, 0x145ea9f0f3b41a9e, 0x57d5ce2a9505c21b),
    "kitti 1241x376 L8 sf1.2 B64 mode0 ORBX_QT_SORTED=0": (0x2b990db2be2f7677, 0x145ea9f0f3b41a9e, 0x57d5ce2a9505c21b),
}


def _digest(case, mode, env, monkeypatch):
    from orb_slam_cuda_amd._lib import OrbxConfig
    for k in ("ORBX_QT_GENERIC", "ORBX_QT_SORTED", "ORBX_QT_LDS_KB", "ORBX_PYR_PADMOD", "ORBX_PYR_KEEP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # the planner reads its switches per call
    _, W, H, nl, sf, B = case
    f = pkg.lib().orbx_plan_digest
    f.argtypes = [C.POINTER(OrbxConfig), C.POINTER(C.c_ulonglong)]
    cfg = OrbxConfig(nfeatures=2000, scale_factor=sf, nlevels=nl, ini_th_fast=20, min_th_fast=7, width=W, height=H,
                     device=0, max_batch=B, scale_mode=mode, pattern_mode=0)
    out = (C.c_ulonglong * 3)()
    assert f(C.byref(cfg), out) == 0, pkg.lib().orbx_last_error()
    return tuple(out)


@pytest.mark.parametrize("case,mode,env", CASES, ids=[_key(*c) for c in CASES])
def test_plan_matches_the_recorded_digests(monkeypatch, case, mode, env):
    got = _digest(case, mode, env, monkeypatch)
    assert got == _digest(case, mode, env, monkeypatch), "two runs of one plan differ"
    assert got == RECORDED[_key(case, mode, env)]


def test_the_switches_change_the_plan():
    """The three KITTI cases are three plans (a switch that was no longer read would go unseen)."""
    d = [RECORDED[_key(KITTI, 0, e)][0] for e in ({}, {"ORBX_QT_GENERIC": "1"}, {"ORBX_QT_SORTED": "0"})]
    assert len(set(d)) == 3


def test_fast_frame_index_magic_is_exact():
    """FAST's frame index (orbx_fast.hip) is mulhi(id, m) with m = ceil(2^32 / d),
    d = cells per frame, which the planner (exact_div_magic, orbx_plan.hip) enables
    only while d * B * (m * d - 2^32) < 2^32. Checked here at the worst ids (the last
    id of each frame, where the remainder is d - 1) for every d the planner can
    produce and the largest B that passes the check, plus a random sample; and the
    planner's helper gives that m at that B and refuses the next B that fails the bound."""
    import numpy as np
    magic = pkg.lib().orbx_exact_div_magic
    magic.argtypes = [C.c_ulonglong, C.c_ulonglong]
    magic.restype = C.c_uint
    rng = np.random.default_rng(7)
    for d in list(range(2, 5001)) + [8191, 12000, 40000]:
        m = ((1 << 32) + d - 1) // d
        e = m * d - (1 << 32)
        bmax = ((1 << 32) - 1) // (d * e) if e else 1 << 20
        if e and bmax >= 1:
            assert magic(d, bmax) == m and magic(d, bmax + 1) == 0, d
        bmax = min(bmax, 1 << 14)
        if bmax < 1:
            assert magic(d, 1) == 0, d
            continue
        assert magic(d, bmax) == m, d
        ids = [(q + 1) * d - 1 for q in range(0, bmax, max(1, bmax // 64))] + [d * bmax - 1]
        ids += [int(x) for x in rng.integers(0, d * bmax, 16)]
        for i in ids:
            assert (i * m) >> 32 == i // d, (d, bmax, i)
    assert magic(0, 1) == 0 and magic(1, 64) == 0  # no cells, one cell: the kernel divides
