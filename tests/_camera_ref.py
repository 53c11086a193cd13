"""Float64 yardstick of tn_camera_rays: the lens models as the header defines them, iterated to convergence (50 Newton
iterations), plus the FORWARD distortion, which the kernel never evaluates -- so ``distort(undistort(p)) == p`` is an independent check
that a fixture lens is invertible where it is used.  tests/test_nerfstudio_abi.py pins this file; the GPU tests compare against it.

A lens is the 10 numbers of tn_camera_table.lens: fx fy cx cy k1 k2 k3 k4 p1 p2.  Models: 0 pinhole, 1 OpenCV, 2 OpenCV fisheye."""
import numpy as np

PINHOLE, OPENCV, FISHEYE = 0, 1, 2
ITERS = 50
W, H = 1296, 968          # the image the fixture lenses were checked on


def lens(f, k=(0., 0., 0., 0.), p=(0., 0.), w=W, h=H, cx=None, cy=None):
    return np.array([f, f, 0.5 * w if cx is None else cx, 0.5 * h if cy is None else cy, *k, *p], dtype=np.float64)


# (model, lens): invertible on the whole 1296 x 968 image (round trip <= 4e-16 in normalised coordinates)
FIXTURES = {
    "opencv_a": (OPENCV, lens(800., (-0.12, 0.03, -0.004, 0.0005), (8e-4, -6e-4))),        # corner shift 85 px
    "opencv_b": (OPENCV, lens(900., (0.10, 0.02, 0., 0.), (-1e-3, 7e-4))),                 # 49 px
    "opencv_c": (OPENCV, lens(1000., (0.05, -0.02, 0., 0.), (1e-3, -5e-4))),
    "fisheye": (FISHEYE, lens(420., (-0.03, 0.005, -0.002, 0.0003))),                      # theta_d up to 1.92
    "pinhole": (PINHOLE, lens(1111.1111)),
}
# NOT invertible towards the corners of that image (the round trip misses by 0.16 and more): only for the "finite and unit length" test
NOT_INVERTIBLE = (OPENCV, lens(700., (-0.28, 0.09, -0.012, 0.), (0., 0.)))


def scaled(model_lens, w, h):
    """the same lens on a w x h image: focal and centre scaled with the width, so that the field of view -- and with it the part of
    the distortion curve in use -- stays inside what the fixture was checked on (h / w must not exceed 968 / 1296)"""
    model, L = model_lens
    assert h * W <= H * w + W
    out = L.copy()
    out[:2] *= w / W
    out[2], out[3] = 0.5 * w, 0.5 * h
    return model, out


def normalised(L, u, v):
    """pixel (u, v) -> (xd, yd): pixel centres at +0.5, image axes (y down)"""
    return (np.asarray(u, np.float64) + 0.5 - L[2]) / L[0], (np.asarray(v, np.float64) + 0.5 - L[3]) / L[1]


def distort(model, L, x, y):
    """forward model: undistorted (x, y) -- the direction (x, -y, -1); fisheye: theta (cos phi, sin phi) -- -> distorted normalised (xd, yd)"""
    k1, k2, k3, k4, p1, p2 = L[4:]
    if model == PINHOLE:
        return x, y
    if model == OPENCV:
        r2 = x * x + y * y
        rad = 1. + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3 + k4 * r2 ** 4
        return x * rad + 2. * p1 * x * y + p2 * (r2 + 2. * x * x), y * rad + 2. * p2 * x * y + p1 * (r2 + 2. * y * y)
    th = r = np.sqrt(x * x + y * y)             # fisheye: (x, y) = theta (cos phi, sin phi) -- theta passes pi / 2 on the fixture, tan would not do
    thd = th * (1. + k1 * th ** 2 + k2 * th ** 4 + k3 * th ** 6 + k4 * th ** 8)
    s = np.where(r > 0, thd / np.where(r > 0, r, 1.), 1.)
    return x * s, y * s


def undistort(model, L, xd, yd, iters=ITERS):
    """(xd, yd) -> undistorted (x, y), the direction (x, -y, -1); fisheye: theta (cos phi, sin phi)"""
    xd, yd = np.asarray(xd, np.float64), np.asarray(yd, np.float64)
    if model == PINHOLE:
        return xd, yd
    if model == FISHEYE:
        th, td = fisheye_theta(L, xd, yd, iters)
        s = np.where(td > 0, th / np.where(td > 0, td, 1.), 1.)
        return xd * s, yd * s
    k1, k2, k3, k4, p1, p2 = L[4:]
    x, y = xd.copy(), yd.copy()
    for _ in range(iters):
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        rad = 1. + r2 * (k1 + r2 * (k2 + r2 * (k3 + r2 * k4)))
        dr = k1 + r2 * (2. * k2 + r2 * (3. * k3 + r2 * 4. * k4))
        f1 = x * rad + 2. * p1 * xy + p2 * (r2 + 2. * xx) - xd
        f2 = y * rad + 2. * p2 * xy + p1 * (r2 + 2. * yy) - yd
        j11 = rad + 2. * xx * dr + 2. * p1 * y + 6. * p2 * x
        j12 = 2. * xy * dr + 2. * p1 * x + 2. * p2 * y
        j22 = rad + 2. * yy * dr + 2. * p2 * x + 6. * p1 * y
        det = j11 * j22 - j12 * j12
        x, y = x - (j22 * f1 - j12 * f2) / det, y - (j11 * f2 - j12 * f1) / det
    return x, y


def fisheye_theta(L, xd, yd, iters=ITERS):
    k1, k2, k3, k4 = L[4:8]
    td = np.sqrt(xd * xd + yd * yd)
    th = td.copy()
    for _ in range(iters):
        t2 = th * th
        f = th * (1. + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - td
        df = 1. + t2 * (3. * k1 + t2 * (5. * k2 + t2 * (7. * k3 + t2 * 9. * k4)))
        th = th - f / df
    return th, td


def camera_dirs(model, L, u, v):
    """direction of pixel (u, v) in the camera frame (x right, y up, looking down -z): [..., 3]; unit length for the fisheye only"""
    xd, yd = normalised(L, u, v)
    if model == FISHEYE:
        th, td = fisheye_theta(L, xd, yd)
        s = np.where(td > 0, np.sin(th) / np.where(td > 0, td, 1.), 1.)
        return np.stack([xd * s, -yd * s, -np.cos(th)], -1)
    x, y = undistort(model, L, xd, yd)
    return np.stack([x, -y, -np.ones_like(x)], -1)


def rays(c2w, model, L, u, v):
    """world rays of pixels (u, v) of one camera: origins [..., 3] (the translation column), unit directions [..., 3]"""
    c2w = np.asarray(c2w, np.float64)
    d = camera_dirs(model, L, u, v) @ c2w[:3, :3].T
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return np.broadcast_to(c2w[:3, 3], d.shape).copy(), d


def table_rays(c2w, models, lenses, sizes, g):
    """the rays of flat pixels `g` of a table of cameras (sizes [n, 2] = w h; row-major inside an image, images in order)"""
    sizes = np.asarray(sizes, np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes[:, 0] * sizes[:, 1])])
    g = np.asarray(g, np.int64)
    assert g.min() >= 0 and g.max() < offsets[-1]
    img = np.searchsorted(offsets, g, side="right") - 1
    o, d = np.zeros((g.size, 3)), np.zeros((g.size, 3))
    for i in np.unique(img):
        sel = img == i
        p = g[sel] - offsets[i]
        o[sel], d[sel] = rays(c2w[i], int(models[i]), np.asarray(lenses[i], np.float64), p % sizes[i, 0], p // sizes[i, 0])
    return o, d, img


def round_trip_error(model, L, w, h, step=1):
    """largest |distort(undistort(p)) - p| over the pixels of a w x h image (every `step`-th, corners and edges always), in
    normalised coordinates"""
    us = np.unique(np.concatenate([np.arange(0, w, step), [w - 1]]))
    vs = np.unique(np.concatenate([np.arange(0, h, step), [h - 1]]))
    u, v = np.meshgrid(us, vs, indexing="xy")
    xd, yd = normalised(L, u, v)
    x, y = undistort(model, L, xd, yd)
    bx, by = distort(model, L, x, y)
    return max(np.abs(bx - xd).max(), np.abs(by - yd).max())
