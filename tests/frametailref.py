"""The tail of the reference's Frame constructors restated in numpy,
independently of the library: Frame::UndistortKeyPoints (src/Frame.cc:403-433),
Frame::ComputeImageBounds (:435-463), Frame::ComputeStereoFromRGBD (:642-663)
and the depth image's convertTo of Tracking::GrabImageRGBD
(src/Tracking.cc:276-277, factor from :150-154).

cv::undistortPoints(src, dst, K, dist, Mat(), K) is the OpenCV 3.x scalar
loop: float inputs widened to double, five fixed-point iterations without an
early exit or an icdist guard, one float rounding at the end. Every operation
here is one numpy float64 / float32 operation (numpy rounds each to nearest
and fuses nothing), so host, device and this file must agree bit for bit."""
import numpy as np

f32, f64 = np.float32, np.float64

# Camera.* of the reference's Examples/*.yaml: fx, fy, cx, cy | k1, k2, p1, p2[, k3]
EUROC = ((458.654, 457.296, 367.215, 248.375), (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05))
TUM1 = ((517.306408, 516.469215, 318.643040, 255.313989), (0.262383, -0.953104, -0.005358, 0.002628, 1.163314))
TUM3 = ((535.4, 539.2, 320.1, 247.6), (0.0, 0.0, 0.0, 0.0))
QUIRK = (TUM1[0], (0.0, 0.1, 0.01, 0.0))  # k1 == 0 with other coefficients set: still "no distortion"
TUM1_BF, TUM1_DEPTH_MAP_FACTOR = 40.0, 5000.0


def K_of(cal):
    fx, fy, cx, cy = cal[0]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)


def dist_of(cal):
    return np.array(cal[1], f32)


def _coeffs(cal):
    fx, fy, cx, cy = (f64(f32(v)) for v in cal[0])
    k = [f64(f32(v)) for v in cal[1]] + [f64(0)] * (5 - len(cal[1]))
    return fx, fy, cx, cy, k


def undistort_points(cal, xy):
    """cv::undistortPoints for (n, 2) float32 points -> (n, 2) float32."""
    fx, fy, cx, cy, k = _coeffs(cal)
    xy = np.asarray(xy, f32).reshape(-1, 2)
    u, v = xy[:, 0].astype(f64), xy[:, 1].astype(f64)
    one, two = f64(1), f64(2)
    with np.errstate(all="ignore"):
        ifx, ify = one / fx, one / fy
        x0 = (u - cx) * ifx
        y0 = (v - cy) * ify
        x, y = x0, y0
        for _ in range(5):
            r2 = x * x + y * y
            icdist = one / (one + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            dX = two * k[2] * x * y + k[3] * (r2 + two * x * x)
            dY = k[2] * (r2 + two * y * y) + two * k[3] * x * y
            x = (x0 - dX) * icdist
            y = (y0 - dY) * icdist
        out = np.stack([(fx * x + cx).astype(f32), (fy * y + cy).astype(f32)], 1)
    return out


def undistort_keypoints(cal, kps):
    """Frame::UndistortKeyPoints: a copy when k1 == 0.0f, else pt replaced."""
    out = kps.copy()
    if f32(cal[1][0]) == f32(0):
        return out
    xy = undistort_points(cal, np.stack([kps["x"], kps["y"]], 1))
    out["x"], out["y"] = xy[:, 0], xy[:, 1]
    return out


def image_bounds(cal, w, h):
    """Frame::ComputeImageBounds -> (mnMinX, mnMaxX, mnMinY, mnMaxY) float32."""
    if f32(cal[1][0]) != f32(0):
        c = undistort_points(cal, np.array([[0, 0], [w, 0], [0, h], [w, h]], f32))
        return (min(c[0, 0], c[2, 0]), max(c[1, 0], c[3, 0]), min(c[0, 1], c[1, 1]), max(c[2, 1], c[3, 1]))
    return (f32(0), f32(w), f32(0), f32(h))


def depth_map_factor(yaml_value):
    """mDepthMapFactor (src/Tracking.cc:150-154) from the yaml's DepthMapFactor."""
    f = f32(yaml_value)
    return f32(1) if abs(float(f)) < 1e-5 else f32(1) / f


def stereo_from_rgbd(kps, kps_un, depth_img, factor, mbf):
    """GrabImageRGBD's convertTo then ComputeStereoFromRGBD: (mvuRight, mvDepth).
    factor = mDepthMapFactor (float32). An index outside the image (undefined
    in the reference) gives -1."""
    factor, mbf = f32(factor), f32(mbf)
    img = np.asarray(depth_img)
    convert = bool(np.abs(factor - f32(1)) > f32(1e-5)) or img.dtype != np.float32
    n = len(kps)
    uright = np.full(n, -1, f32)
    depth = np.full(n, -1, f32)
    h, w = img.shape
    with np.errstate(all="ignore"):
        for i in range(n):
            iu, iv = int(kps["x"][i]), int(kps["y"][i])  # truncation, as Mat::at<float>(float, float)
            if not (0 <= iu < w and 0 <= iv < h):
                continue
            d = f32(img[iv, iu])
            if convert:
                d = f32(d * factor)
            if d > 0:
                depth[i] = d
                uright[i] = f32(kps_un["x"][i] - f32(mbf / d))
    return uright, depth
