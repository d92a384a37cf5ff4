"""Frame::isInFrustum (src/Frame.cc:268-324) restated in numpy, independently of
the library: every reference operation is one float32 or float64 numpy
operation (numpy rounds each to nearest and fuses nothing), in the order and
precision cv::Mat gives them:

* Pc = mRcw*P + mtcw: gemm's small-matrix path, a float dot product and a
  double add of t;
* invz = 1.0f/PcZ and u = fx*PcX*invz + cx in float, left to right;
* mOw = -mRcw.t()*mtcw: the general gemm path, a double sum times -1.0;
* cv::norm: the square root of the double sum of squares, to float;
* PO.dot(Pn)/dist: Mat::dot in double, a double divide, one rounding to float;
* PredictScale from the oracle (O.predict_scale).

The comparisons keep the reference's form, so a NaN passes them as it does
there. Records are the library's 24-byte orbm_map_point_proj; a point that is
not tested or not in view is all zero apart from obs_positive."""
import numpy as np

f32, f64 = np.float32, np.float64

# why a point left isInFrustum (REASONS[code])
NOT_VALID, BEHIND, OUTSIDE_IMAGE, DISTANCE, VIEW_ANGLE, IN_VIEW = range(6)
REASONS = ("not valid", "behind the camera", "outside the image", "outside the distance band", "viewing angle",
           "in view")


def camera_centre(Tcw):
    """mOw = -mRcw.t()*mtcw (Frame::UpdatePoseMatrices, src/Frame.cc:260-266)."""
    T = np.asarray(Tcw, f32).reshape(-1)[:12].reshape(3, 4)
    ow = np.zeros(3, f32)
    for r in range(3):
        s = f64(0)
        for k in range(3):
            s = s + f64(T[k, r]) * f64(T[k, 3])
        ow[r] = f32(s * f64(-1.0))
    return ow


def is_in_frustum(O, proj_dtype, fx, fy, cx, cy, mbf, Tcw, bounds, scale_factor, nlevels, limit, mps):
    """(records, reason codes) for the orbm_map_point_world records mps."""
    T = np.asarray(Tcw, f32).reshape(-1)[:12].reshape(3, 4)
    fx, fy, cx, cy, mbf, limit = f32(fx), f32(fy), f32(cx), f32(cy), f32(mbf), f32(limit)
    minX, maxX, minY, maxY = (f32(b) for b in bounds)
    N = len(mps)
    out = np.zeros(N, proj_dtype)
    out["obs_positive"] = mps["obs_positive"]
    why = np.full(N, IN_VIEW, np.int32)
    P = np.ascontiguousarray(mps["pos"], f32)
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        def row(r):
            t = (T[r, 0] * X + T[r, 1] * Y) + T[r, 2] * Z
            return (t.astype(f64) + f64(T[r, 3])).astype(f32)
        xc, yc, zc = row(0), row(1), row(2)
        invz = f32(1.0) / zc
        u = (fx * xc) * invz + cx
        v = (fy * yc) * invz + cy
        maxd = f32(1.2) * mps["max_distance"].astype(f32)
        mind = f32(0.8) * mps["min_distance"].astype(f32)
        ow = camera_centre(T)
        PO = [X - ow[0], Y - ow[1], Z - ow[2]]
        d = [p.astype(f64) for p in PO]
        dist = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).astype(f32)
        nrm = np.ascontiguousarray(mps["normal"], f32).astype(f64)
        dot = (d[0] * nrm[:, 0] + d[1] * nrm[:, 1]) + d[2] * nrm[:, 2]
        view_cos = (dot / dist.astype(f64)).astype(f32)
        xr = u - mbf * invz
        # the reference's early returns, the last applied first so that the first one wins
        why[view_cos < limit] = VIEW_ANGLE
        why[(dist < mind) | (dist > maxd)] = DISTANCE
        why[(u < minX) | (u > maxX) | (v < minY) | (v > maxY)] = OUTSIDE_IMAGE
        why[zc < f32(0.0)] = BEHIND
        why[mps["valid"] == 0] = NOT_VALID
    ok = why == IN_VIEW
    for j in np.nonzero(ok)[0]:
        out["predicted_level"][j] = O.predict_scale(float(mps["max_distance"][j]), float(dist[j]),
                                                    float(scale_factor), int(nlevels))
    out["proj_x"][ok] = u[ok]
    out["proj_y"][ok] = v[ok]
    out["proj_xr"][ok] = xr[ok]
    out["view_cos"][ok] = view_cos[ok]
    out["track_in_view"][ok] = 1
    return out, why


def scene_frustum(O, proj_dtype, c, limit=0.5):
    """is_in_frustum for a frustumcase scene."""
    return is_in_frustum(O, proj_dtype, c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"], c["Tcw"], c["bounds"],
                         c["scale_factor"], c["nlevels"], limit, c["mps"])


def local_points(O, proj_dtype, c, th, nnratio, limit=0.5):
    """Tracking::SearchLocalPoints on a frustumcase scene: isInFrustum above, then the oracle's
    SearchByProjection(F, vpMapPoints, th) over all the records. (out, nmatches, records, n_in_view)."""
    proj, why = scene_frustum(O, proj_dtype, c, limit)
    out, nm = O.search_by_projection(c["kps"], c["desc"], c["uright"], c["bounds"], c["scale"], c["blocked"],
                                     proj.view(O.MP_DTYPE), c["mpdesc"], th, nnratio)
    return out, nm, proj, int((why == IN_VIEW).sum())
