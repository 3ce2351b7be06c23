"""The contract of spt_temporal_* (include/smallpt_mi355x.h) restated in numpy float32: vectorised over pixels, explicit Python loops over
the four taps in the stated order (dy outer, dx inner).  Every operation is one float32 operation on float32 operands, so each rounds
once; no np.sum / np.dot / einsum (their summation order is not the contract's).  The camera inverse is restated in float64 with the
cofactor sequence of the header.  Test infrastructure: the GPU tests compare the library with it bit for bit."""
import numpy as np

F = np.float32
SMALLPT, PINHOLE = 0, 1


class Params:
    def __init__(self, alpha=0.1, max_len=32.0, tau_normal=0.5, tau_plane=10.0):
        self.alpha, self.max_len, self.tau_normal, self.tau_plane = F(alpha), F(max_len), F(tau_normal), F(tau_plane)

    @classmethod
    def of(cls, p):
        """From anything with the four fields (the package's TemporalParams, the ctypes struct)."""
        return cls(p.alpha, p.max_len, p.tau_normal, p.tau_plane)


class Camera:
    """origin, dir, cx, cy (float32 triples), push (float32), sampler -- of anything with those fields (the package's SptCamera)."""
    def __init__(self, cam):
        self.origin, self.dir, self.cx, self.cy = (np.array([float(v) for v in getattr(cam, k)], dtype=F) for k in ("origin", "dir", "cx", "cy"))
        self.push = F(cam.push)
        self.sampler = int(cam.sampler)

    def equals(self, o):
        """Every field compares equal as floats and the samplers match (NaN never compares equal)."""
        return bool(all((getattr(self, k) == getattr(o, k)).all() for k in ("origin", "dir", "cx", "cy")) and self.push == o.push
                    and self.sampler == o.sampler)


def camera_inverse(cam):
    """(3, 3) float32 W, or None when the contract rejects the camera."""
    a = np.stack([cam.cx, cam.cy, cam.dir], axis=1).astype(np.float64)       # columns cx, cy, dir
    if not np.isfinite(a).all():
        return None
    adj = np.empty((3, 3))
    adj[0][0] = a[1][1] * a[2][2] - a[1][2] * a[2][1]
    adj[0][1] = a[0][2] * a[2][1] - a[0][1] * a[2][2]
    adj[0][2] = a[0][1] * a[1][2] - a[0][2] * a[1][1]
    adj[1][0] = a[1][2] * a[2][0] - a[1][0] * a[2][2]
    adj[1][1] = a[0][0] * a[2][2] - a[0][2] * a[2][0]
    adj[1][2] = a[0][2] * a[1][0] - a[0][0] * a[1][2]
    adj[2][0] = a[1][0] * a[2][1] - a[1][1] * a[2][0]
    adj[2][1] = a[0][1] * a[2][0] - a[0][0] * a[2][1]
    adj[2][2] = a[0][0] * a[1][1] - a[0][1] * a[1][0]
    det = (a[0][0] * adj[0][0] + a[0][1] * adj[1][0]) + a[0][2] * adj[2][0]
    if det == 0.0 or det != det:
        return None
    with np.errstate(all="ignore"):
        w = (adj / det).astype(F)
    return w if np.isfinite(w).all() else None


def lum(v):
    return (F(0.2126) * v[..., 0] + F(0.7152) * v[..., 1]) + F(0.0722) * v[..., 2]


def guides(normal, position, coverage):
    """n, x (h, w, 3) and c (h, w): N / c and P / c where c > 0, else 0."""
    c = np.ascontiguousarray(coverage, dtype=F)[..., 0]
    hit = c > 0
    safe = np.where(hit, c, F(1))[..., None]
    with np.errstate(all="ignore"):
        n, x = (np.where(hit[..., None], np.asarray(s, dtype=F) / safe, F(0)).astype(F) for s in (normal, position))
    return n, x, c


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def step(frame, normal, position, coverage, frame_samples, cam, prev_cam, hist, p, info=None):
    """One step.  frame, normal, position, coverage: (h, w, 3) float32 sums; hist: the (3, h, w, 4) history of the previous step or None;
    cam, prev_cam: Camera (prev_cam may be None without a history).  Returns (history' (3, h, w, 4), rgb (h, w, 3), var (h, w), len (h, w),
    has (h, w) bool: the pixel found a history).  A dict passed as ``info`` receives what the tests assert about their own inputs: 'mode'
    and, for a reprojection, 'behind' (c > 0 but q.z <= push), 'off' (projected outside the range test), 'inside' and 'taps' (per pixel:
    taps inside the image, taps that passed every test)."""
    frame = np.ascontiguousarray(frame, dtype=F)
    h, w = frame.shape[:2]
    with np.errstate(all="ignore"):
        ws = F(1) / F(frame_samples)
        cur = frame * ws
        lc = lum(cur)
        m2c = lc * lc
        n, x, c = guides(normal, position, coverage)
        has = np.zeros((h, w), dtype=bool)
        hv = np.zeros((h, w, 5), dtype=F)                                   # mean r, g, b, len, m2
        if hist is not None:
            hist = np.ascontiguousarray(hist, dtype=F)
            assert hist.shape == (3, h, w, 4)
            if cam.equals(prev_cam):                                        # the identity rule: the stored values, no arithmetic
                hv[..., :4] = hist[0]
                hv[..., 4] = hist[2][..., 3]
                has[:] = True
                if info is not None:
                    info["mode"] = "identity"
            else:
                W = camera_inverse(prev_cam)
                assert W is not None, "the previous camera has no inverse: the library refuses the call"
                v = x - prev_cam.origin
                q = [(W[i][0] * v[..., 0] + W[i][1] * v[..., 1]) + W[i][2] * v[..., 2] for i in range(3)]
                ok = (c > 0) & (q[2] > prev_cam.push)
                front = ok.copy()
                ax, ay = q[0] / q[2], q[1] / q[2]
                if prev_cam.sampler == SMALLPT:
                    ux, uy = ax + F(0.5), ay + F(0.5)
                else:
                    ux, uy = (ax + F(1)) * F(0.5), (ay + F(1)) * F(0.5)
                sx, sy = ux * F(w) - F(0.5), uy * F(h) - F(0.5)
                ok &= (F(-1) <= sx) & (sx < F(w)) & (F(-1) <= sy) & (sy < F(h))       # in float, before any conversion; NaN fails
                sx, sy = np.where(ok, sx, F(0)), np.where(ok, sy, F(0))
                x0f, y0f = np.floor(sx), np.floor(sy)
                fx, fy = sx - x0f, sy - y0f
                x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
                num = np.zeros((h, w, 5), dtype=F)
                wsum = np.zeros((h, w), dtype=F)
                n_inside, n_taps = np.zeros((h, w), dtype=int), np.zeros((h, w), dtype=int)
                for dy in (0, 1):
                    for dx in (0, 1):
                        tx, ty = x0 + dx, y0 + dy
                        inside = ok & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
                        txc, tyc = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)
                        t0, t1, t2 = hist[0][tyc, txc], hist[1][tyc, txc], hist[2][tyc, txc]
                        valid = inside & (t1[..., 3] > 0)
                        en = _sq3(n - t1[..., :3])
                        d = t2[..., :3] - x
                        pl = (n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]
                        ep = pl * pl
                        valid &= (en <= p.tau_normal) & (ep <= p.tau_plane)
                        wt = (fx if dx else F(1) - fx) * (fy if dy else F(1) - fy)
                        assert wt.dtype == F and en.dtype == F and ep.dtype == F
                        vals = (t0[..., 0], t0[..., 1], t0[..., 2], t0[..., 3], t2[..., 3])
                        for k in range(5):
                            num[..., k] = np.where(valid, num[..., k] + wt * vals[k], num[..., k])
                        wsum = np.where(valid, wsum + wt, wsum)
                        n_inside += inside
                        n_taps += valid
                if info is not None:
                    info.update(mode="reproject", behind=(c > 0) & ~front, off=front & ~ok, inside=n_inside, taps=n_taps)
                has = wsum > 0
                hv = np.where(has[..., None], num / np.where(has, wsum, F(1))[..., None], F(0)).astype(F)
        elif info is not None:
            info["mode"] = "none"
        t = hv[..., 3] + F(1)
        length = np.where(t < p.max_len, t, p.max_len).astype(F)
        r = F(1) / length
        a = np.where(p.alpha > r, p.alpha, r).astype(F)
        rgb = hv[..., :3] + a[..., None] * (cur - hv[..., :3])
        m2 = hv[..., 4] + a * (m2c - hv[..., 4])
        rgb = np.where(has[..., None], rgb, cur).astype(F)
        m2 = np.where(has, m2, m2c).astype(F)
        length = np.where(has, length, F(1)).astype(F)
        lo = lum(rgb)
        var = m2 - lo * lo
        var = np.where(var > 0, var, F(0)).astype(F)
    out = np.empty((3, h, w, 4), dtype=F)
    out[0][..., :3], out[0][..., 3] = rgb, length
    out[1][..., :3], out[1][..., 3] = n, c
    out[2][..., :3], out[2][..., 3] = x, m2
    assert rgb.dtype == F and var.dtype == F and length.dtype == F
    return out, rgb, var, length, has


def run(frames, cams, p, resets=()):
    """The loop: frames = [(frame, normal, position, coverage, frame_samples)], cams = [Camera]; resets = indices of frames that drop the
    history.  Returns the list of step() results."""
    hist, prev, res = None, None, []
    for i, (f, cam) in enumerate(zip(frames, cams)):
        if i in resets:
            hist = None
        r = step(f[0], f[1], f[2], f[3], f[4], cam, prev, hist, p)
        res.append(r)
        hist, prev = r[0], cam
    return res


class PlainCamera:
    """A camera from arrays, with the fields Camera() reads and as_c() for the library."""
    def __init__(self, origin, dir, cx, cy, push, sampler):
        self.origin, self.dir, self.cx, self.cy, self.push, self.sampler = origin, dir, cx, cy, push, sampler

    def as_c(self, pkg):
        cam = pkg.SptCamera()
        for k in ("origin", "dir", "cx", "cy"):
            getattr(cam, k)[:] = [float(v) for v in getattr(self, k)]
        cam.push = float(self.push)
        cam.sampler = int(self.sampler)
        return cam


def project(cam, pts, w, h):
    """Continuous pixel coordinates (sx, sy) of world points under a Camera, in float64: for building test inputs only."""
    a = np.stack([cam.cx, cam.cy, cam.dir], axis=1).astype(np.float64)
    q = (np.asarray(pts, dtype=np.float64) - cam.origin.astype(np.float64)) @ np.linalg.inv(a).T
    ax, ay = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
    ux, uy = (ax + 0.5, ay + 0.5) if cam.sampler == SMALLPT else ((ax + 1) * 0.5, (ay + 1) * 0.5)
    return ux * w - 0.5, uy * h - 0.5


def unproject(cam, sx, sy, depth, w, h):
    """World points o + depth * (cx*ax + cy*ay + dir) of continuous pixel coordinates, float64: for building test inputs only."""
    ux, uy = (np.asarray(sx, dtype=np.float64) + 0.5) / w, (np.asarray(sy, dtype=np.float64) + 0.5) / h
    ax, ay = (ux - 0.5, uy - 0.5) if cam.sampler == SMALLPT else (2 * ux - 1, 2 * uy - 1)
    d = cam.cx.astype(np.float64) * ax[..., None] + cam.cy.astype(np.float64) * ay[..., None] + cam.dir.astype(np.float64)
    return cam.origin.astype(np.float64) + np.asarray(depth, dtype=np.float64)[..., None] * d


def _base_camera(w, h, sampler):
    """A camera 250 in front of the wall z = 0, looking along -z: the smallpt kind (push 140) or the pinhole kind (push 0)."""
    if sampler == SMALLPT:
        return PlainCamera(np.array([50, 52, 250], dtype=F), np.array([0, 0, -1], dtype=F), np.array([F(0.5135 * w / h), 0, 0], dtype=F),
                           np.array([0, 0.5135, 0], dtype=F), F(140), SMALLPT)
    return PlainCamera(np.array([50, 52, 250], dtype=F), np.array([0, 0, -1], dtype=F), np.array([0.4, 0, 0], dtype=F),
                       np.array([0, 0.3, 0], dtype=F), F(0), PINHOLE)


def _wall_points(cam, sx, sy, w, h):
    """Where the camera's rays through continuous pixel coordinates meet the wall z = 0 (float32, z exactly 0)."""
    one = unproject(cam, sx, sy, np.ones_like(np.asarray(sx, dtype=np.float64)), w, h) - cam.origin.astype(np.float64)     # the ray direction d
    t = -cam.origin.astype(np.float64)[2] / one[..., 2]
    pts = (cam.origin.astype(np.float64) + t[..., None] * one).astype(F)
    pts[..., 2] = F(0)
    return pts


def moved_camera(base, w, h, move):
    """'same', 'translate' (a few pixels sideways and a step forward) or 'rotate' (about the y and z axes) of a base camera."""
    o, d, cx, cy = (getattr(base, k).astype(np.float64) for k in ("origin", "dir", "cx", "cy"))
    if move == "same":
        return PlainCamera(base.origin.copy(), base.dir.copy(), base.cx.copy(), base.cy.copy(), base.push, base.sampler)
    px = (2.3 if w >= 5 else 0.3) * 250 * np.linalg.norm(cx) * (1 if base.sampler == SMALLPT else 2) / w     # world size of that many pixels
    py = (1.4 if h >= 3 else 0.2) * 250 * np.linalg.norm(cy) * (1 if base.sampler == SMALLPT else 2) / h
    if move == "translate":
        return PlainCamera((o + [px, -py, -3.0]).astype(F), base.dir.copy(), base.cx.copy(), base.cy.copy(), base.push, base.sampler)
    assert move == "rotate"
    a, b = px / 250, 0.02                                                    # about y by `a`, about z by `b`
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    r = ry @ rz
    return PlainCamera(base.origin.copy(), (r @ d).astype(F), (r @ cx).astype(F), (r @ cy).astype(F), base.push, base.sampler)


PROBES = [(-0.6, 3.3), (-0.6, -0.6), (3.3, -0.6), (-1.0, 2.0), (-1.4, 2.0), (2.0, -1.4)]      # plus their mirror images at the far edges


def synthetic(w, h, sampler, move, seed):
    """Inputs of one step on a wall z = 0 with normal (0, 0, 1), exactly representable, seen by a previous camera and a moved one.
    History: means over several orders of magnitude, lengths 1 .. 7, three vertical bands -- A as the wall, B with normal (0.5, 0, 1)
    (en = 0.25 exactly against the wall's), C at z = 0.5 (ep = 0.25 exactly) --, scattered pixels with c = 0, with NaN normals and with
    NaN points.  Frame: the wall through the moved camera with hit counts 1, 2, 4 (exact guides), 3, and 0; pixels in front of the camera
    but within push, and behind it; NaN guides; and probe pixels whose point projects just off each edge and corner of the previous image.
    Returns a dict: prev_cam, cam (PlainCamera), hist, frame, normal, position, coverage, samples."""
    rng = np.random.default_rng(seed)
    base = _base_camera(w, h, sampler)
    cam = moved_camera(base, w, h, move)
    yy, xx = np.mgrid[0:h, 0:w]
    # the previous history
    hist = np.zeros((3, h, w, 4), dtype=F)
    hist[0][..., :3] = (10.0 ** rng.uniform(-3, 2, (h, w, 3))).astype(F)
    hist[0][..., 3] = rng.choice(np.array([1, 2, 2.5, 7], dtype=F), (h, w))
    band = (xx * 3) // max(w, 1)
    hist[1][..., :3] = np.where((band == 1)[..., None], np.array([0.5, 0, 1], dtype=F), np.array([0, 0, 1], dtype=F))
    hist[1][..., 3] = rng.choice(np.array([1, 2, 3, 4], dtype=F), (h, w))
    hist[2][..., :3] = _wall_points(base, xx, yy, w, h)
    hist[2][..., 2] = np.where(band == 2, F(0.5), F(0))
    hist[2][..., 3] = (10.0 ** rng.uniform(-4, 3, (h, w))).astype(F)
    u = rng.random((h, w))
    if w * h > 4:
        hist[1][..., 3][u < 0.08] = F(0)
        hist[1][..., 0][(u >= 0.08) & (u < 0.11)] = np.nan
        hist[2][..., 1][(u >= 0.11) & (u < 0.14)] = np.nan
    # the frame
    samples = 4
    frame = (10.0 ** rng.uniform(-3, 2, (h, w, 3))).astype(F) * F(samples)
    c = rng.choice(np.array([1, 2, 4, 3, 0], dtype=F), (h, w), p=[0.3, 0.25, 0.25, 0.1, 0.1])
    if w * h <= 4:
        c[:] = F(2)
    x = _wall_points(cam, xx, yy, w, h)
    n = np.broadcast_to(np.array([0, 0, 1], dtype=F), (h, w, 3)).copy()
    v = rng.random((h, w))
    if w * h > 4:
        x[v < 0.04] = (cam.origin.astype(np.float64) + [1.0, 2.0, -50.0]).astype(F)      # in front, within a push of 140
        x[(v >= 0.04) & (v < 0.08)] = (base.origin.astype(np.float64) + [3.0, 1.0, 8.0]).astype(F)   # behind the previous camera
        n[(v >= 0.08) & (v < 0.10), 1] = np.nan
        x[(v >= 0.10) & (v < 0.12), 0] = np.nan
        x[(v >= 0.12) & (v < 0.16), 2] = F(0.25)                                         # off the wall by less than tau_plane allows
    if w * h >= 40:
        probes = PROBES + [(w - 1 - a, h - 1 - b) for a, b in PROBES]
        for i, (sx, sy) in enumerate(probes):
            k = (5 + 7 * i) % (w * h)
            py, px = divmod(k, w)
            x[py, px] = _wall_points(base, np.array(sx), np.array(sy), w, h)
            n[py, px] = (0, 0, 1)
            c[py, px] = F(1)
    mult = np.where(c > 0, c, F(3))[..., None]                                           # pixels without hits keep non-zero sums
    normal, position = (n * mult).astype(F), (x * mult).astype(F)
    coverage = np.repeat(c[..., None], 3, axis=-1).astype(F)
    return dict(prev_cam=base, cam=cam, hist=hist, frame=frame, normal=normal, position=position, coverage=coverage, samples=samples)


def moving_camera(pkg, w, h, step, i):
    """The smallpt camera of a w x h image with its origin moved by i steps (float32 adds of the float32 products)."""
    cam = pkg.smallpt_camera(w, h)
    for k in range(3):
        cam.origin[k] = float(F(cam.origin[k]) + F(step[k] * i))
    return cam


def oracle_sequence(pkg, step, w=64, h=48, samps=1, nframes=8, ref_samps=64, ref_seed=11):
    """Cornell-9 on the CPU: per frame i (seed i, the camera moved by i steps) the oracle's un-normalised render and the feature sums of
    tests/aov_set_expected.py as step() takes them; the Cameras; and a normalised ref_samps render from the last camera (float64)."""
    import aov_set_expected as aset
    import oracle_binding as orc
    scene = pkg.cornell9()
    frames = []
    for i in range(nframes):
        cam = moving_camera(pkg, w, h, step, i)
        beauty, _ = orc.render(scene, w, h, samps, seed=i, camera=orc.camera_from(cam))
        g, _ = aset.all_kinds(lambda r: aset.sphere_hits(scene, r), scene["color"], w, h, samps, i, cam)
        frames.append((beauty, g["normal"][0], g["position"][0], g["coverage"][0], 4 * samps))
    ref, _ = orc.render(scene, w, h, ref_samps, seed=ref_seed, normalise=True, camera=orc.camera_from(moving_camera(pkg, w, h, step, nframes - 1)))
    return frames, [Camera(moving_camera(pkg, w, h, step, i)) for i in range(nframes)], ref.astype(np.float64)


def rel_l2(img, ref):
    return float(np.sqrt(((np.asarray(img, dtype=np.float64) - ref) ** 2).sum()) / np.sqrt((ref ** 2).sum()))
