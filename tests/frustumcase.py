"""Synthetic scenes for Frame::isInFrustum and Tracking::SearchLocalPoints: a
frame extracted by the oracle, a pose, and local map points built as posecase
builds them for Fuse (back-projected from the keypoints, some behind the camera
or off the image, distances around the keypoint's octave with 5 % outside the
scale-invariance band, unit normals along the viewing ray, 6 % of them
flipped). On top of that 60 % of the normals are tilted by 0-70 degrees about
random axes: untilted, every in-view cosine is above 0.998 and
RadiusByViewingCos' 4.0 branch (src/ORBmatcher.cc:120-126) never runs; tilted,
the cosines spread over both branches and past the 0.5 limit. Points without
observations, duplicated points racing for one keypoint and pre-blocked
keypoints exercise the search's sequential blocking (a point with observations
blocks its keypoint for the points after it, so the smaller obs_frac, the later
the points that still get a keypoint)."""
import numpy as np

from posecase import CX, CY, FX, FY, MB, _distances, _dups, _frame, _noisy, _points, pose, rodrigues


def frustum_case(O, seed, W=320, H=240, nf=300, nmp=600, stereo=False, sf=1.2, L=8, obs_frac=0.85):
    kps, desc, scale = _frame(O, seed, W, H, nf)
    rng = np.random.default_rng(7000 + seed)
    Tcw = pose(rng)
    src, near, Xw, z = _points(rng, kps, Tcw, nmp, W, H, px_noise=1.2)
    mps = np.zeros(nmp, O.MPW_DTYPE)
    mps["pos"] = Xw
    d = _distances(rng, mps, Xw, Tcw, src, near, kps, sf, L)
    Ow = np.linalg.inv(Tcw)[:3, 3]
    nrm = (Xw - Ow) / d[:, None]
    flip = rng.random(nmp) < 0.06
    nrm = np.where(flip[:, None], -nrm, nrm)
    tilt = rng.random(nmp) < 0.6
    ang = np.radians(rng.uniform(0.0, 70.0, nmp))
    axis = rng.normal(0, 1, (nmp, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    for j in np.nonzero(tilt)[0]:
        nrm[j] = rodrigues(axis[j] * ang[j]) @ nrm[j]
    mps["normal"] = nrm.astype(np.float32)
    mps["valid"] = rng.random(nmp) < 0.9
    mps["obs_positive"] = rng.random(nmp) < obs_frac
    mpd = np.where(near[:, None], _noisy(rng, desc[src], 0.06), rng.integers(0, 256, (nmp, 32))).astype(np.uint8)
    _dups(rng, mps, mpd, 0.1)
    n = len(kps)
    uright = None
    if stereo:
        zk = rng.uniform(2.0, 45.0, n)
        zk[src[near]] = z[near]
        uright = np.where(rng.random(n) < 0.6, kps["x"] - FX * MB / zk + rng.normal(0, 0.8, n), -1.0).astype(np.float32)
    blocked = (rng.random(n) < 0.1).astype(np.uint8)
    return dict(kps=kps, desc=desc, uright=uright, bounds=(0.0, float(W), 0.0, float(H)),
                scale=np.asarray(scale, np.float32), scale_factor=sf, nlevels=L, blocked=blocked, fx=FX, fy=FY, cx=CX,
                cy=CY, mb=MB, mbf=MB * FX, Tcw=Tcw[:3].astype(np.float32), mps=mps, mpdesc=mpd)
