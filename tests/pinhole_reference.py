"""CPU expectation for the pinhole distortion models (plumb_bob, radtan, rational_polynomial): a numpy / Python-float
restatement of PARITY.md "Pinhole distortion models" in the stated operation order.  Python floats and numpy float64 are IEEE
doubles, every product and sum is rounded on its own (no contraction), so the results can be compared with ``==``.

``new_camera_matrix`` / ``maps``: the contract, statement for statement.  ``maps_independent``: a second evaluation that
shares nothing with it but the formula of the model -- vectorised, np.linalg.inv, no row accumulation -- to catch a formula
restated wrongly on both sides (agreement within 1e-3 px, not bit for bit)."""
import numpy as np

PINHOLE_MODELS = ("plumb_bob", "radtan", "rational_polynomial")

# name -> (model, D): the calibrations of the tests.  With K of synth.pinhole_camera_model they are invertible over the field
# of view at every size used (a k3 = -0.03 variant of barrel+k3 folds over and must not be used).
CALIBRATIONS = {
    "barrel": ("plumb_bob", [-0.28, 0.07, 2e-4, -3e-4, 0.0]),
    "barrel+k3": ("plumb_bob", [-0.25, 0.08, 1e-3, -5e-4, -0.01]),
    "pincushion": ("radtan", [0.12, 0.02, -4e-4, 6e-4]),
    "rational": ("rational_polynomial", [0.9, 0.25, 3e-4, -2e-4, 0.01, 1.25, 0.55, 0.05]),
}
MAP_SIZES = ((31, 9), (32, 16), (33, 17), (65, 33), (200, 136))  # on and around the 32-pixel chunk and the 64 x 16 tile


def coefficients(model, D):
    """(k1, k2, p1, p2, k3, k4, k5, k6) as the model evaluates them: missing values are 0, radtan has no k3, only
    rational_polynomial keeps k4..k6."""
    n = {"plumb_bob": 5, "radtan": 4, "rational_polynomial": 8}[model]
    d = [float(v) for v in D][:n]
    return d + [0.0] * (8 - len(d))


def reported_count(model):
    return {"plumb_bob": 5, "radtan": 5, "rational_polynomial": 8}.get(model, 4)


def mul3(a, b):
    """rip_host.cpp mul3: row times column, three products summed left to right."""
    return [a[i * 3 + 0] * b[0 * 3 + j] + a[i * 3 + 1] * b[1 * 3 + j] + a[i * 3 + 2] * b[2 * 3 + j] for i in range(3) for j in range(3)]


def inverse3(a):
    """rip_host.cpp inverse3: adjugate times 1 / det."""
    c0 = a[4] * a[8] - a[5] * a[7]
    c1 = a[5] * a[6] - a[3] * a[8]
    c2 = a[3] * a[7] - a[4] * a[6]
    inv_det = 1.0 / (a[0] * c0 + a[1] * c1 + a[2] * c2)
    return [c0 * inv_det, (a[2] * a[7] - a[1] * a[8]) * inv_det, (a[1] * a[5] - a[2] * a[4]) * inv_det,
            c1 * inv_det, (a[0] * a[8] - a[2] * a[6]) * inv_det, (a[2] * a[3] - a[0] * a[5]) * inv_det,
            c2 * inv_det, (a[1] * a[6] - a[0] * a[7]) * inv_det, (a[0] * a[4] - a[1] * a[3]) * inv_det]


def new_camera_matrix(K, model, D, size, balance, new_size=None, fov_scale=1.0):
    """cv::getOptimalNewCameraMatrix with alpha = balance clamped to [0, 1], in Python floats; 3 x 3 float64."""
    K = [float(v) for v in np.asarray(K, np.float64).ravel()]
    k1, k2, p1, p2, k3, k4, k5, k6 = coefficients(model, D)
    w, h = int(size[0]), int(size[1])
    nw, nh = (int(new_size[0]), int(new_size[1])) if new_size else (w, h)
    balance = min(max(float(balance), 0.0), 1.0)
    px = [[0.0] * 9 for _ in range(9)]
    py = [[0.0] * 9 for _ in range(9)]
    for gy in range(9):
        for gx in range(9):
            u, v = gx * float(w - 1) / 8, gy * float(h - 1) / 8
            x0, y0 = (u - K[2]) / K[0], (v - K[5]) / K[4]
            x, y = x0, y0
            for _ in range(20):
                r2 = x * x + y * y
                icd = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
                dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
                dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
                x = (x0 - dx) * icd
                y = (y0 - dy) * icd
            px[gy][gx], py[gy][gx] = x, y
    inner = (max(px[a][0] for a in range(9)), min(px[a][8] for a in range(9)),
             max(py[0][a] for a in range(9)), min(py[8][a] for a in range(9)))
    flat_x = [px[a][b] for a in range(9) for b in range(9)]
    flat_y = [py[a][b] for a in range(9) for b in range(9)]
    outer = (min(flat_x), max(flat_x), min(flat_y), max(flat_y))

    def camera(left, right, top, bottom):
        fx, fy = (nw - 1) / (right - left), (nh - 1) / (bottom - top)
        return fx, fy, -fx * left, -fy * top

    fx, fy, cx, cy = [a * (1 - balance) + b * balance for a, b in zip(camera(*inner), camera(*outer))]
    if fov_scale > 0:
        fx, fy = fx / fov_scale, fy / fov_scale
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], np.float64)


def maps(K, model, D, R, P, size):
    """cv::initUndistortRectifyMap (CV_32FC1) in double, rows accumulated with np.add.accumulate; (map_x, map_y) float32."""
    K = [float(v) for v in np.asarray(K, np.float64).ravel()]
    R = [float(v) for v in np.asarray(R, np.float64).ravel()]
    P = [float(v) for v in np.asarray(P, np.float64).reshape(3, -1)[:, :3].ravel()]
    k1, k2, p1, p2, k3, k4, k5, k6 = coefficients(model, D)
    w, h = int(size[0]), int(size[1])
    iR = inverse3(mul3(P, R))
    fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    i = np.arange(h, dtype=np.float64)

    def walk(step, a, b):
        start = i * a + b
        seq = np.empty((h, w), np.float64)
        seq[:, 0] = start
        seq[:, 1:] = step
        return np.add.accumulate(seq, axis=1)  # X_j = (((X_0 + s) + s) + ...) + s, one rounding per column

    X, Y, W = walk(iR[0], iR[1], iR[2]), walk(iR[3], iR[4], iR[5]), walk(iR[6], iR[7], iR[8])
    with np.errstate(all="ignore"):
        wi = 1.0 / W
        x, y = X * wi, Y * wi
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        xy2 = 2 * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + p1 * xy2 + p2 * (r2 + 2 * x2)
        yd = y * kr + p1 * (r2 + 2 * y2) + p2 * xy2
        return (fx * xd + cx).astype(np.float32), (fy * yd + cy).astype(np.float32)


def maps_independent(K, model, D, R, P, size):
    """The same maps from the definition of the model: every pixel back-projected through inv(P R) on its own, radial and
    tangential terms in their textbook form.  float64."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    P = np.asarray(P, np.float64).reshape(3, -1)[:, :3]
    k1, k2, p1, p2, k3, k4, k5, k6 = coefficients(model, D)
    w, h = int(size[0]), int(size[1])
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    rays = np.linalg.inv(P @ R) @ np.stack([u.ravel(), v.ravel(), np.ones(w * h)])
    x, y = rays[0] / rays[2], rays[1] / rays[2]
    r2 = x ** 2 + y ** 2
    radial = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x ** 2)
    yd = y * radial + p1 * (r2 + 2 * y ** 2) + 2 * p2 * x * y
    return (K[0, 0] * xd + K[0, 2]).reshape(h, w), (K[1, 1] * yd + K[1, 2]).reshape(h, w)


def inside_share(mx, my, size):
    """Share of the destination pixels whose map entry lies inside the w x h source."""
    w, h = size
    with np.errstate(invalid="ignore"):
        return float(((mx >= 0) & (mx <= w - 1) & (my >= 0) & (my <= h - 1)).mean())


def check_map_conditions(mx, my, size, balance, what=""):
    """What every frame test asserts on its own maps, so that it never compares black with black: at least half of the
    destination samples inside the source and, at balance 1, at least 3 % outside."""
    share = inside_share(mx, my, size)
    assert share >= 0.5, "%s: only %.3f of the destination pixels sample inside the source" % (what, share)
    if balance == 1:
        assert 1 - share >= 0.03, "%s: only %.3f of the destination pixels fall outside at balance 1" % (what, 1 - share)
    return share


def rotation_y(angle):
    c, s = float(np.cos(angle)), float(np.sin(angle))
    return [c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c]


def load(pipe, name, size, balance=0.0, fov_scale=1.0, R=None):
    """Loads calibration `name` at `size` through the YAML loader; returns (cam, model)."""
    from raw_image_pipeline_amd import synth
    model, D = CALIBRATIONS[name]
    cam = synth.pinhole_camera_model(size[0], size[1], D)
    if R is not None:
        cam["R"] = list(R)
    synth.load_camera(pipe, cam, model)
    pipe.set_undistortion_balance(balance)
    pipe.set_undistortion_fov_scale(fov_scale)
    return cam, model


def reference_maps(pipe, cam, model):
    """The reference maps for the handle's own new camera matrix (so that a map comparison does not depend on it)."""
    size = (cam["width"], cam["height"])
    return maps(cam["K"], model, cam["D"], cam["R"], pipe.get_rect_camera_matrix(), size)
