"""Host-side mirror of the reference's render interface on top of the C-ABI.

``Renderer.render`` plays the role of ``Renderer::render`` (smallpt.cpp:692-814, un-normalised sum,
row 0 = bottom) and ``Renderer.cpu_render_equivalent`` that of ``cpuRender`` (smallpt.cpp:269-379,
normalised).  PyTorch is only used for device memory / streams when the caller wants the image to
stay resident in HBM.
"""
import ctypes as C

import numpy as np

from ._lib import SptCamera, SptDemodParams, SptDenoiseParams, SptDenoiseVarParams, SptDisplayParams, SptInstance, SptMaterial, SptMesh, SptMultiStats, SptStats, SptTemporalParams, SptTemporalVarParams, load_library, load_multi_library
from .scene import HIT_DTYPE, INSTANCE_DTYPE, PATH_DTYPE, RAY_DTYPE, RAY_RANGE_DTYPE, SPHERE_DTYPE

FLAG_NORMALISE = 1
FLAG_ONE_SHOT = 2          # scheduling only: no dispatch order used or recorded for this launch (include/smallpt_mi355x.h)
ACCEL_EXHAUSTIVE, ACCEL_BVH, ACCEL_GRID, ACCEL_BVH_FAST, ACCEL_AUTO = 0, 1, 2, 3, 4


def _ray_array(rays):
    """RAY_DTYPE[n], or floats of shape (n, 6), as a contiguous RAY_DTYPE array; anything else is refused."""
    a = np.asarray(rays)
    if a.dtype == RAY_DTYPE:
        if a.ndim != 1:
            raise ValueError(f"rays: expected a 1-D array of RAY_DTYPE, got shape {a.shape}")
        return np.ascontiguousarray(a)
    if a.dtype.fields is not None or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"rays: expected RAY_DTYPE or real numbers, got dtype {a.dtype}")
    if a.ndim != 2 or a.shape[1] != 6:
        raise ValueError(f"rays: expected shape (n, 6), got {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float32).view(RAY_DTYPE).reshape(-1)


def _range_array(who, rays):
    """RAY_RANGE_DTYPE[n], or floats of shape (n, 8) {o, tmin, d, tmax}, as a contiguous RAY_RANGE_DTYPE array; anything else is refused."""
    a = np.asarray(rays)
    if a.dtype == RAY_RANGE_DTYPE:
        if a.ndim != 1:
            raise ValueError(f"{who}: expected a 1-D array of RAY_RANGE_DTYPE, got shape {a.shape}")
        return np.ascontiguousarray(a)
    if a.dtype.fields is not None or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"{who}: expected RAY_RANGE_DTYPE or real numbers, got dtype {a.dtype}")
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError(f"{who}: expected rays of shape (n, 8) {{o, tmin, d, tmax}}, got {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float32).view(RAY_RANGE_DTYPE).reshape(-1)


def _range_host(r, who, name, rays):
    """Renderer.trace_spheres_range / trace_rays_range: the rays are checked before the library is called."""
    rays = _range_array(who, rays)
    n = len(rays)
    hits = np.zeros(n, dtype=HIT_DTYPE)
    r._check(getattr(r._lib, name)(r._h, rays.ctypes.data_as(C.c_void_p), n, hits.ctypes.data_as(C.c_void_p)))
    return hits


def _range_device(r, who, name, rays_t, hits_t, stream):
    """Renderer.trace_spheres_range_device / trace_rays_range_device: the same, for device tensors."""
    import torch
    if not (isinstance(rays_t, torch.Tensor) and rays_t.is_cuda and rays_t.dtype == torch.float32 and rays_t.is_contiguous()
            and rays_t.dim() == 2 and rays_t.shape[1] == 8 and rays_t.data_ptr() % 16 == 0):
        raise ValueError(f"{who}: rays_t must be a contiguous, 16-byte aligned float32 device tensor of shape (n, 8)")
    n = rays_t.shape[0]
    if hits_t is None:
        hits_t = torch.empty((n, 11), dtype=torch.float32, device=rays_t.device)
    elif not (isinstance(hits_t, torch.Tensor) and hits_t.device == rays_t.device and hits_t.dtype == torch.float32
              and hits_t.is_contiguous() and tuple(hits_t.shape) == (n, 11)):
        raise ValueError(f"{who}: hits_t must be a contiguous float32 tensor of shape (n, 11) on the rays' device")
    fn = getattr(r._lib, name)
    stream = stream if stream is not None else torch.cuda.current_stream(rays_t.device)
    if stream.cuda_stream == 0:
        # handle 0 would be the context's own stream, not ordered with torch's default one: as trace_spheres_device
        side = torch.cuda.Stream(rays_t.device)
        side.wait_stream(stream)
        r._check(fn(r._h, C.c_void_p(rays_t.data_ptr()), n, C.c_void_p(hits_t.data_ptr()), C.c_void_p(side.cuda_stream)))
        stream.wait_stream(side)
        return hits_t
    r._check(fn(r._h, C.c_void_p(rays_t.data_ptr()), n, C.c_void_p(hits_t.data_ptr()), C.c_void_p(stream.cuda_stream)))
    return hits_t


def _occluded_host(r, who, name, rays, tmax):
    """Renderer.occluded_spheres / occluded_rays: every argument is checked before the library is called."""
    rays = _ray_array(rays)
    n = len(rays)
    tm = None
    if tmax is not None:
        tm = np.asarray(tmax)
        if not (np.issubdtype(tm.dtype, np.floating) or np.issubdtype(tm.dtype, np.integer)) or tm.shape != (n,):
            raise ValueError(f"{who}: tmax must be real numbers of shape ({n},), got dtype {tm.dtype} and shape {tm.shape}")
        tm = np.ascontiguousarray(tm, dtype=np.float32)
    out = np.zeros(n, dtype=np.bool_)
    r._check(getattr(r._lib, name)(r._h, rays.ctypes.data_as(C.c_void_p), tm.ctypes.data_as(C.c_void_p) if tm is not None else None, n,
                                   out.ctypes.data_as(C.c_void_p)))
    return out


def _occluded_device(r, who, name, rays_t, tmax_t, out_t, stream):
    """Renderer.occluded_spheres_device / occluded_rays_device: the same, for device tensors."""
    import torch
    if not (isinstance(rays_t, torch.Tensor) and rays_t.is_cuda and rays_t.dtype == torch.float32 and rays_t.is_contiguous()
            and rays_t.dim() == 2 and rays_t.shape[1] == 6):
        raise ValueError(f"{who}: rays_t must be a contiguous float32 device tensor of shape (n, 6)")
    n = rays_t.shape[0]
    if tmax_t is not None and not (isinstance(tmax_t, torch.Tensor) and tmax_t.device == rays_t.device and tmax_t.dtype == torch.float32
                                   and tmax_t.is_contiguous() and tuple(tmax_t.shape) == (n,)):
        raise ValueError(f"{who}: tmax_t must be a contiguous float32 tensor of shape (n,) on the rays' device")
    if out_t is None:
        out_t = torch.empty(n, dtype=torch.bool, device=rays_t.device)
    elif not (isinstance(out_t, torch.Tensor) and out_t.device == rays_t.device and out_t.dtype == torch.bool
              and out_t.is_contiguous() and tuple(out_t.shape) == (n,)):
        raise ValueError(f"{who}: out_t must be a contiguous torch.bool tensor of shape (n,) on the rays' device")
    fn = getattr(r._lib, name)
    tp = C.c_void_p(tmax_t.data_ptr()) if tmax_t is not None else None
    stream = stream if stream is not None else torch.cuda.current_stream(rays_t.device)
    if stream.cuda_stream == 0:
        # handle 0 would be the context's own stream, not ordered with torch's default one: as trace_spheres_device
        side = torch.cuda.Stream(rays_t.device)
        side.wait_stream(stream)
        r._check(fn(r._h, C.c_void_p(rays_t.data_ptr()), tp, n, C.c_void_p(out_t.data_ptr()), C.c_void_p(side.cuda_stream)))
        stream.wait_stream(side)
        return out_t
    r._check(fn(r._h, C.c_void_p(rays_t.data_ptr()), tp, n, C.c_void_p(out_t.data_ptr()), C.c_void_p(stream.cuda_stream)))
    return out_t


def _wf_tensor(who, t, dtype, rows, cols):
    """A device tensor of the wavefront entries: contiguous, of ``dtype``, shape (>= rows, cols)."""
    if not (hasattr(t, "data_ptr") and t.device.type == "cuda" and str(t.dtype) == dtype and t.is_contiguous() and t.dim() == 2
            and t.shape[1] == cols and t.shape[0] >= rows):
        raise ValueError(f"{who}: expected a contiguous {dtype} device tensor of shape (>= {rows}, {cols})")


# spt_render_aov kinds (include/smallpt_mi355x.h SPT_AOV_*)
AOV_KINDS = {"normal": 0, "albedo": 1, "uv": 2, "dist": 3}


# spt_render_aov_set kinds: bit k of the mask (SPT_AOVSET_* = 1 << k); the four above, the hit point and the hit count
AOV_SET_KINDS = dict(AOV_KINDS, position=4, coverage=5)


def _aov_set(kinds):
    """(mask, the selected names in ascending bit order) of an iterable of AOV_SET_KINDS names."""
    if isinstance(kinds, str):
        kinds = (kinds,)
    try:
        names = list(kinds)
    except TypeError:
        raise ValueError(f"kinds must be an iterable of names out of {', '.join(AOV_SET_KINDS)}") from None
    for k in names:
        if not isinstance(k, str) or k not in AOV_SET_KINDS:
            raise ValueError(f"unknown aov {k!r}: one of {', '.join(AOV_SET_KINDS)}")
    if not names:
        raise ValueError("kinds is empty")
    if len(set(names)) != len(names):
        raise ValueError("kinds names a buffer twice")
    names.sort(key=AOV_SET_KINDS.get)
    return sum(1 << AOV_SET_KINDS[k] for k in names), names


# SPT_AOV_EMISSION: a kind of the single-kind entries only (no set bit), so it is in neither table above
AOV_EMISSION = 6


def _aov_kind(aov):
    if aov == "emission":
        return AOV_EMISSION
    if not isinstance(aov, str) or aov not in AOV_KINDS:
        raise ValueError(f"unknown aov {aov!r}: one of {', '.join(AOV_KINDS)}, emission")
    return AOV_KINDS[aov]


class DenoiseParams:
    """Parameters of the edge-avoiding wavelet filter (spt_denoise_params): ``levels`` passes (1..5, pass i at step 2^i pixels) and the four
    edge-stopping strengths, each finite and >= 0.  Anything left None takes the library's default (spt_denoise_params_default);
    ``sigma_plane`` is in 1/(scene length)^2 and the default suits the Cornell box's scale of about 100."""
    FIELDS = ("levels", "sigma_normal", "sigma_plane", "sigma_albedo", "sigma_coverage")

    def __init__(self, levels=None, sigma_normal=None, sigma_plane=None, sigma_albedo=None, sigma_coverage=None):
        c = SptDenoiseParams()
        load_library().spt_denoise_params_default(C.byref(c))
        given = (levels, sigma_normal, sigma_plane, sigma_albedo, sigma_coverage)
        for name, v in zip(self.FIELDS, given):
            setattr(self, name, getattr(c, name) if v is None else (int(v) if name == "levels" else float(v)))

    def as_c(self):
        c = SptDenoiseParams()
        for name in self.FIELDS:
            setattr(c, name, getattr(self, name))
        return c

    def __repr__(self):
        return "DenoiseParams(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.FIELDS) + ")"


def _denoise_params(params):
    return (params if params is not None else DenoiseParams()).as_c()


class DenoiseVarParams:
    """Parameters of the variance-guided filter (spt_denoise_var_params): those of ``DenoiseParams`` and ``sigma_colour`` (finite, >= 0),
    the strength of the luminance edge-stopping term; 0 gives ``denoise`` bit for bit.  None takes spt_denoise_var_params_default."""
    FIELDS = DenoiseParams.FIELDS + ("sigma_colour",)

    def __init__(self, levels=None, sigma_normal=None, sigma_plane=None, sigma_albedo=None, sigma_coverage=None, sigma_colour=None):
        c = SptDenoiseVarParams()
        load_library().spt_denoise_var_params_default(C.byref(c))
        given = (levels, sigma_normal, sigma_plane, sigma_albedo, sigma_coverage, sigma_colour)
        for name, v in zip(self.FIELDS, given):
            setattr(self, name, getattr(c, name) if v is None else (int(v) if name == "levels" else float(v)))

    def as_c(self):
        c = SptDenoiseVarParams()
        for name in self.FIELDS:
            setattr(c, name, getattr(self, name))
        return c

    def __repr__(self):
        return "DenoiseVarParams(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.FIELDS) + ")"


def _denoise_var_params(params):
    return (params if params is not None else DenoiseVarParams()).as_c()


DISPLAY_RGB8, DISPLAY_RGBA8 = 0, 1
DISPLAY_FLIP_Y = 1
DISPLAY_SRC_ACCUM, DISPLAY_SRC_DENOISED, DISPLAY_SRC_DENOISED_VAR = 0, 1, 2


class DisplayParams:
    """Parameters of the 8-bit display transform (spt_display_params): ``weight`` (one number or three, each finite and >= 0: the
    reference's 1/(sampleCount*sampleCountPerPixel)), ``format`` 'rgb8' or 'rgba8' (alpha = 255) and ``flip_y`` (top row first, the order
    of a PPM body; default bottom row first, GL's order).  Defaults as spt_display_params_default: weight 1, rgb8, no flip."""
    FORMATS = {"rgb8": DISPLAY_RGB8, "rgba8": DISPLAY_RGBA8}

    def __init__(self, weight=None, format="rgb8", flip_y=False):
        c = SptDisplayParams()
        load_library().spt_display_params_default(C.byref(c))
        if weight is None:
            self.weight = tuple(float(v) for v in c.weight)
        else:
            wt = np.atleast_1d(np.asarray(weight, dtype=np.float32))
            if wt.shape not in ((1,), (3,)):
                raise ValueError("DisplayParams: weight is one number or three")
            self.weight = tuple(float(v) for v in np.broadcast_to(wt, (3,)))
        self.format = self.FORMATS[format] if isinstance(format, str) else int(format)
        self.flags = DISPLAY_FLIP_Y if flip_y is True else int(flip_y)

    @property
    def channels(self):
        return 4 if self.format == DISPLAY_RGBA8 else 3

    def as_c(self):
        c = SptDisplayParams()
        c.weight[:] = self.weight
        c.format = self.format
        c.flags = self.flags
        return c

    def __repr__(self):
        return f"DisplayParams(weight={self.weight!r}, format={self.format!r}, flags={self.flags!r})"


def _display_params(params):
    return params if params is not None else DisplayParams()


class TemporalParams:
    """Parameters of the temporal accumulation (spt_temporal_params): ``alpha`` in [0, 1], the lower bound of the current frame's weight
    (0 = the running mean up to ``max_len``); ``max_len`` >= 1, the cap of the per-pixel history length; ``tau_normal`` and ``tau_plane``
    >= 0, the largest squared normal difference and squared distance from the pixel's tangent plane -- in (scene length)^2 -- at which a
    history tap still counts.  Anything left None takes the library's default (spt_temporal_params_default: 0.1, 32, 0.5, 10)."""
    FIELDS = ("alpha", "max_len", "tau_normal", "tau_plane")

    def __init__(self, alpha=None, max_len=None, tau_normal=None, tau_plane=None):
        c = SptTemporalParams()
        load_library().spt_temporal_params_default(C.byref(c))
        for name, v in zip(self.FIELDS, (alpha, max_len, tau_normal, tau_plane)):
            setattr(self, name, getattr(c, name) if v is None else float(v))

    def as_c(self):
        c = SptTemporalParams()
        for name in self.FIELDS:
            setattr(c, name, getattr(self, name))
        return c

    def __repr__(self):
        return "TemporalParams(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.FIELDS) + ")"


def _temporal_params(params):
    return (params if params is not None else TemporalParams()).as_c()


class TemporalVarParams:
    """Parameters of the variance estimate from a temporal history (spt_temporal_var_params): ``min_len`` >= 1, the history length below
    which a pixel takes the 7 x 7 spatial estimate instead of its own temporal variance; ``sigma_normal`` and ``sigma_plane`` >= 0, the
    strengths of the squared normal difference and of the squared distance from the pixel's tangent plane in a spatial tap's weight.
    Anything left None takes the library's default (spt_temporal_var_params_default: 4, 32, 0.2)."""
    FIELDS = ("min_len", "sigma_normal", "sigma_plane")

    def __init__(self, min_len=None, sigma_normal=None, sigma_plane=None):
        c = SptTemporalVarParams()
        load_library().spt_temporal_var_params_default(C.byref(c))
        for name, v in zip(self.FIELDS, (min_len, sigma_normal, sigma_plane)):
            setattr(self, name, getattr(c, name) if v is None else float(v))

    def as_c(self):
        c = SptTemporalVarParams()
        for name in self.FIELDS:
            setattr(c, name, getattr(self, name))
        return c

    def __repr__(self):
        return "TemporalVarParams(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.FIELDS) + ")"


def _temporal_var_params(params):
    return (params if params is not None else TemporalVarParams()).as_c()


class DemodParams:
    """Parameters of albedo demodulation (spt_demod_params): ``albedo_floor`` >= 0, the mean albedo at or below which a channel passes
    through undivided, and ``background`` (one number or three, >= 0), the environment radiance of escaped paths -- pass
    ``Renderer.environment()``.  Anything left None takes the library's default (spt_demod_params_default: 1/64 and 0)."""

    def __init__(self, albedo_floor=None, background=None):
        c = SptDemodParams()
        load_library().spt_demod_params_default(C.byref(c))
        self.albedo_floor = float(c.albedo_floor) if albedo_floor is None else float(albedo_floor)
        if background is None:
            self.background = tuple(float(v) for v in c.background)
        else:
            bg = np.atleast_1d(np.asarray(background, dtype=np.float32))
            if bg.shape not in ((1,), (3,)):
                raise ValueError("DemodParams: background is one number or three")
            self.background = tuple(float(v) for v in np.broadcast_to(bg, (3,)))

    def as_c(self):
        c = SptDemodParams()
        c.albedo_floor = self.albedo_floor
        c.background[:] = self.background
        return c

    def __repr__(self):
        return f"DemodParams(albedo_floor={self.albedo_floor!r}, background={self.background!r})"


def _demod_params(params):
    return (params if params is not None else DemodParams()).as_c()


def temporal_history_bytes(w, h):
    """Size of one history of the temporal accumulation: three float4 planes, 48 bytes per pixel (spt_temporal_history_bytes)."""
    return int(load_library().spt_temporal_history_bytes(int(w), int(h)))


def camera_inverse(camera):
    """(3, 3) float32: the inverse of the matrix with columns cx, cy, dir of ``camera`` (spt_camera_inverse), computed in double and rounded
    once; ValueError when the library rejects it (a singular or non-finite camera)."""
    out = np.empty((3, 3), dtype=np.float32)
    if load_library().spt_camera_inverse(C.byref(camera), out.ctypes.data_as(C.c_void_p)):
        raise ValueError("camera_inverse: the camera's {cx | cy | dir} has no inverse")
    return out


class SptError(RuntimeError):
    pass


def instance_records(instances):
    """INSTANCE_DTYPE[n] from a sequence of (model, 3x4 matrix), an INSTANCE_DTYPE array or ((n, 12) float32, (n,) ints)."""
    if isinstance(instances, np.ndarray) and instances.dtype == INSTANCE_DTYPE:
        return np.ascontiguousarray(instances)
    if isinstance(instances, tuple) and len(instances) == 2 and np.asarray(instances[0]).ndim == 2:
        mats, models = np.asarray(instances[0], dtype=np.float32).reshape(-1, 12), np.asarray(instances[1]).reshape(-1)
    else:
        pairs = list(instances)
        mats = np.array([np.asarray(a, dtype=np.float32).reshape(12) for _, a in pairs], dtype=np.float32).reshape(-1, 12)
        models = np.array([int(m) for m, _ in pairs], dtype=np.int64)
    if len(mats) != len(models):
        raise ValueError("instances: one model index per matrix")
    if np.any(models < 0) or np.any(models > 0xFFFFFFFF):
        raise ValueError("instances: model index out of range")
    out = np.zeros(len(mats), dtype=INSTANCE_DTYPE)
    out["transform"] = mats
    out["model"] = models.astype(np.uint32)
    return out


def smallpt_camera(w, h):
    """Camera constants of cpuRender (smallpt.cpp:277-279) for a w x h image."""
    lib = load_library()
    cam = SptCamera()
    if lib.spt_camera_smallpt(w, h, C.byref(cam)):
        raise SptError("spt_camera_smallpt failed")
    return cam


def pinhole_camera(vx=(1, 0, 0), vy=None, vz=(0, 0, -1), org=(0, -1, 0), near=1.0):
    """Camera{vx, vy, vz, org, nearPlaneDistance} of the interactive driver (smallpt.cpp:607-624); the defaults
    are main()'s values (:885-888,899), vy = normalize(cross(vx, vz))."""
    lib = load_library()
    f = np.float32
    if vy is None:
        a, b = np.asarray(vx, dtype=f), np.asarray(vz, dtype=f)
        c = np.array([f(a[1] * b[2]) - f(a[2] * b[1]), f(a[2] * b[0]) - f(a[0] * b[2]), f(a[0] * b[1]) - f(a[1] * b[0])], dtype=f)
        q = f(f(c[0] * c[0]) + f(c[1] * c[1])) + f(c[2] * c[2])
        vy = c * (f(1) / np.sqrt(f(q)))
    cam = SptCamera()
    v3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    if lib.spt_camera_pinhole(v3(vx), v3(vy), v3(vz), v3(org), float(near), C.byref(cam)):
        raise SptError("spt_camera_pinhole failed")
    return cam


def _stats_dict(st):
    return {"samples": int(st.samples), "bounces": int(st.bounces), "max_depth_kills": int(st.max_depth_kills),
            "kernel_ms": float(st.kernel_ms), "finalize_ms": float(st.finalize_ms), "total_ms": float(st.total_ms),
            "grid_blocks": int(st.grid_blocks), "block_threads": int(st.block_threads)}


def environment_radiance(rgb):
    """The radiance E of spt_set_environment as three float32 values: None = black; each component finite and >= 0 (ValueError otherwise,
    before any device call)."""
    if rgb is None:
        return np.zeros(3, dtype=np.float32)
    e = np.asarray(rgb, dtype=np.float64)
    if e.shape != (3,):
        raise ValueError(f"environment: three components (r, g, b) expected, got shape {e.shape}")
    e = e.astype(np.float32)
    if not (np.all(np.isfinite(e)) and np.all(e >= 0)):
        raise ValueError(f"environment: each component must be finite and >= 0, got {e.tolist()}")
    return e


class Renderer:
    """One context = one HIP device (spt_create)."""

    def __init__(self, device_id=0):
        self._lib = load_library()
        h = C.c_void_p()
        if self._lib.spt_create(int(device_id), C.byref(h)):
            raise SptError(self._lib.spt_last_error(None).decode())
        self._h = h
        self.device_id = int(device_id)
        self._scene = None
        # everything a second context needs to render the same frames (ProgressiveRenderer(pipeline=2) replays it on its extra
        # lane): the current scene (sphere table or meshes + materials), the closest-hit modes, tuning and watchdog
        self._state = {"scene": None, "sphere_accel": None, "mesh_accel": None, "tuning": None, "watchdog": None}
        self._state_version = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.spt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc:
            raise SptError(self._lib.spt_last_error(self._h).decode())

    def set_scene(self, spheres):
        spheres = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
        self._scene = spheres
        self._check(self._lib.spt_set_scene(self._h, spheres.ctypes.data_as(C.c_void_p), len(spheres)))
        self._state["scene"] = ("spheres", spheres)
        self._state_version += 1

    def replay_state_on(self, other):
        """Brings another context (same device) to this one's scene, closest-hit modes, tuning and watchdog."""
        st = self._state
        if st["tuning"] is not None:
            other.set_tuning(*st["tuning"])
        if st.get("grid_pools") is not None:
            other.set_grid_pools(*st["grid_pools"])
        if st["watchdog"] is not None:
            other.set_watchdog(st["watchdog"])
        if st["sphere_accel"] is not None:
            other.set_sphere_accel(st["sphere_accel"])
        if st["mesh_accel"] is not None:
            other.set_mesh_accel(st["mesh_accel"])
        if st.get("environment") is not None:
            other.set_environment(st["environment"])
        if st.get("line_form") is not None:
            other.set_line_form(st["line_form"])
        if st["scene"] is not None:
            if st["scene"][0] == "spheres":
                other.set_scene(st["scene"][1])
            elif st["scene"][0] == "instances":
                other.set_instances(st["scene"][1], st["scene"][2], st["scene"][3])
            else:
                other.set_meshes(st["scene"][1], st["scene"][2])

    def set_meshes(self, meshes, materials):
        """Intersector::addTriangleMesh for every TriMesh + build() (smallpt.cpp:437-447); materials[i] = (emission, color,
        refl) of instance i (smallpt.cpp:170).  Makes the mesh scene current for render()."""
        ms = (SptMesh * max(1, len(meshes)))()
        mats = (SptMaterial * max(1, len(meshes)))()
        self._mesh_keepalive = list(meshes)
        for i, (m, (e, col, refl)) in enumerate(zip(meshes, materials)):
            ms[i].positions = m.positions.ctypes.data
            ms[i].normals = m.normals.ctypes.data
            ms[i].indices = m.indices.ctypes.data
            ms[i].nverts, ms[i].ntris = len(m.positions), len(m.indices)
            mats[i].emission = (C.c_float * 3)(*[float(v) for v in e])
            mats[i].color = (C.c_float * 3)(*[float(v) for v in col])
            mats[i].refl = int(refl)
        self._check(self._lib.spt_set_meshes(self._h, ms, len(meshes), mats))
        self._scene = None                                   # the sphere table is no longer the current scene
        self._state["scene"] = ("meshes", list(meshes), list(materials))
        self._state_version += 1

    def set_instances(self, models, instances, materials):
        """rtpModelSetInstances (smallpt.cpp:489-530): models = TriMesh list, instances = a sequence of (model, 3x4 matrix), an
        INSTANCE_DTYPE array, or a pair ((n, 12) float32 matrices, (n,) model indices); materials[i] = (emission, color, refl) of instance i.
        Makes the instanced mesh scene current (include/smallpt_mi355x.h spt_set_instances)."""
        recs = instance_records(instances)
        ms = (SptMesh * max(1, len(models)))()
        for i, m in enumerate(models):
            ms[i].positions, ms[i].normals, ms[i].indices = m.positions.ctypes.data, m.normals.ctypes.data, m.indices.ctypes.data
            ms[i].nverts, ms[i].ntris = len(m.positions), len(m.indices)
        mats = (SptMaterial * max(1, len(materials)))()
        for i, (e, col, refl) in enumerate(materials):
            mats[i].emission = (C.c_float * 3)(*[float(v) for v in e])
            mats[i].color = (C.c_float * 3)(*[float(v) for v in col])
            mats[i].refl = int(refl)
        if len(materials) < len(recs):
            raise ValueError("set_instances: one material per instance")
        self._check(self._lib.spt_set_instances(self._h, ms, len(models), recs.ctypes.data_as(C.POINTER(SptInstance)), len(recs), mats))
        self._mesh_keepalive = list(models)
        self._scene = None
        self._state["scene"] = ("instances", list(models), recs.copy(), list(materials))
        self._state_version += 1

    def set_sphere_accel(self, accel):
        """How sphere tables above 24 spheres find their closest hit: ACCEL_GRID (default: uniform grid in LDS), ACCEL_BVH (hierarchy) --
        both exhaustive-equivalent by construction (include/smallpt_mi355x.h) -- or ACCEL_EXHAUSTIVE."""
        self._check(self._lib.spt_set_sphere_accel(self._h, int(accel)))
        self._state["sphere_accel"] = int(accel)
        self._state_version += 1

    def set_environment(self, rgb):
        """Radiance E gathered by a render path that leaves the scene (smallpt.cpp:168 "path.weight * envContrib"): a miss adds w * E to
        the path's sample.  rgb = (r, g, b), each finite and >= 0; None or (0, 0, 0) = black (the default).  Renders and progressive frames
        only -- not the first-hit feature buffers, not the queries (include/smallpt_mi355x.h spt_set_environment)."""
        e = environment_radiance(rgb)
        self._check(self._lib.spt_set_environment(self._h, e.ctypes.data_as(C.POINTER(C.c_float))))
        self._state["environment"] = e.copy()
        self._state_version += 1

    def environment(self):
        """The context's current E as float32[3]."""
        e = np.zeros(3, dtype=np.float32)
        self._check(self._lib.spt_get_environment(self._h, e.ctypes.data_as(C.POINTER(C.c_float))))
        return e

    def set_mesh_accel(self, accel):
        """ACCEL_AUTO (default: the faster of the two exact modes per launch), ACCEL_BVH (the role of the reference's OptiX Prime model,
        smallpt.cpp:475-603; the exhaustive loop's Hit for every ray, include/smallpt_mi355x.h), ACCEL_EXHAUSTIVE (every triangle, the reference's CPU loops: the parity anchor) or
        ACCEL_BVH_FAST (the plain hierarchy of rounds 2-3 and the thin triangles' lines: faster, but rays lying in a regular triangle's plane to
        rounding may differ)."""
        self._check(self._lib.spt_set_mesh_accel(self._h, int(accel)))
        self._state["mesh_accel"] = int(accel)
        self._state_version += 1

    def trace_rays(self, rays):
        """Intersector::traceRays (smallpt.cpp:460-470): rays = array of RAY_DTYPE (or (n, 6) floats); returns HIT_DTYPE[n]."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6) if not (hasattr(rays, "dtype") and rays.dtype == RAY_DTYPE) else rays
        rays = np.ascontiguousarray(rays)
        n = len(rays)
        hits = np.zeros(n, dtype=HIT_DTYPE)
        self._check(self._lib.spt_trace_rays(self._h, rays.ctypes.data_as(C.c_void_p), n, hits.ctypes.data_as(C.c_void_p)))
        return hits

    def trace_rays_device(self, rays_t, hits_t=None, stream=None):
        """spt_trace_rays_device: rays_t = contiguous float32 CUDA tensor (n, 6) on this renderer's device; returns the float32 tensor
        (n, 11) of Hit records (dist, instId and triId as raw bits, x, n, uv), enqueued on `stream` (a torch stream; default: current)."""
        import torch
        assert rays_t.is_cuda and rays_t.dtype == torch.float32 and rays_t.is_contiguous() and rays_t.shape[-1] == 6
        n = rays_t.numel() // 6
        if hits_t is None:
            hits_t = torch.empty((n, 11), dtype=torch.float32, device=rays_t.device)
        st = (stream if stream is not None else torch.cuda.current_stream(rays_t.device)).cuda_stream
        self._check(self._lib.spt_trace_rays_device(self._h, C.c_void_p(rays_t.data_ptr()), n, C.c_void_p(hits_t.data_ptr()), C.c_void_p(st)))
        return hits_t

    def trace_spheres(self, rays):
        """cpuIntersectGlobalSpheres (smallpt.cpp:144-152) against the current sphere table: rays = RAY_DTYPE[n] or floats of shape (n, 6);
        returns HIT_DTYPE[n] (instId = sphere index, triId = 0, uv = 0; a miss is dist = 1e20 with every other field 0)."""
        rays = _ray_array(rays)
        n = len(rays)
        hits = np.zeros(n, dtype=HIT_DTYPE)
        self._check(self._lib.spt_trace_spheres(self._h, rays.ctypes.data_as(C.c_void_p), n, hits.ctypes.data_as(C.c_void_p)))
        return hits

    def trace_spheres_device(self, rays_t, hits_t=None, stream=None):
        """spt_trace_spheres_device: rays_t = contiguous float32 tensor (n, 6) on this renderer's device; returns the float32 tensor (n, 11)
        of Hit records (dist, instId and triId as raw bits, x, n, uv), enqueued on `stream` (a torch stream; default: the current one)."""
        import torch
        if not (isinstance(rays_t, torch.Tensor) and rays_t.is_cuda and rays_t.dtype == torch.float32 and rays_t.is_contiguous()
                and rays_t.dim() == 2 and rays_t.shape[1] == 6):
            raise ValueError("trace_spheres_device: rays_t must be a contiguous float32 device tensor of shape (n, 6)")
        n = rays_t.shape[0]
        if hits_t is None:
            hits_t = torch.empty((n, 11), dtype=torch.float32, device=rays_t.device)
        elif not (isinstance(hits_t, torch.Tensor) and hits_t.device == rays_t.device and hits_t.dtype == torch.float32
                  and hits_t.is_contiguous() and tuple(hits_t.shape) == (n, 11)):
            raise ValueError("trace_spheres_device: hits_t must be a contiguous float32 tensor of shape (n, 11) on the rays' device")
        stream = stream if stream is not None else torch.cuda.current_stream(rays_t.device)
        if stream.cuda_stream == 0:
            # torch's default stream is handle 0, which the C call reads as "the context's own stream" -- a non-blocking stream not ordered
            # with it: run on a pool stream that waits for the default one, and make the default one wait for the query
            side = torch.cuda.Stream(rays_t.device)
            side.wait_stream(stream)
            self._check(self._lib.spt_trace_spheres_device(self._h, C.c_void_p(rays_t.data_ptr()), n, C.c_void_p(hits_t.data_ptr()),
                                                           C.c_void_p(side.cuda_stream)))
            stream.wait_stream(side)
            return hits_t
        self._check(self._lib.spt_trace_spheres_device(self._h, C.c_void_p(rays_t.data_ptr()), n, C.c_void_p(hits_t.data_ptr()),
                                                       C.c_void_p(stream.cuda_stream)))
        return hits_t

    def occluded_spheres(self, rays, tmax=None):
        """Any-hit queries against the current sphere table (spt_occluded_spheres; OptiX Prime's RTP_QUERY_TYPE_ANY with OptixRay::tmax,
        smallpt.cpp:395-403): rays = RAY_DTYPE[n] or floats (n, 6), tmax = floats (n,) or None (+inf); returns np.bool_[n], True where the
        closest hit of trace_spheres in exhaustive mode has dist < 1e20 and dist < tmax."""
        return _occluded_host(self, "occluded_spheres", "spt_occluded_spheres", rays, tmax)

    def occluded_rays(self, rays, tmax=None):
        """The same against the current mesh scene (spt_occluded_rays: the closest hit of trace_rays in exhaustive mode decides)."""
        return _occluded_host(self, "occluded_rays", "spt_occluded_rays", rays, tmax)

    def occluded_spheres_device(self, rays_t, tmax_t=None, out_t=None, stream=None):
        """spt_occluded_spheres_device: rays_t = contiguous float32 device tensor (n, 6), tmax_t = contiguous float32 tensor (n,) on the same
        device or None (+inf); returns the torch.bool tensor (n,) (out_t if given), enqueued on `stream` (a torch stream; default: the current one)."""
        return _occluded_device(self, "occluded_spheres_device", "spt_occluded_spheres_device", rays_t, tmax_t, out_t, stream)

    def occluded_rays_device(self, rays_t, tmax_t=None, out_t=None, stream=None):
        """spt_occluded_rays_device: as occluded_spheres_device, against the current mesh scene."""
        return _occluded_device(self, "occluded_rays_device", "spt_occluded_rays_device", rays_t, tmax_t, out_t, stream)

    def trace_spheres_range(self, rays):
        """Closest hit inside a per-ray interval against the current sphere table (spt_trace_spheres_range; OptiX Prime's
        RTP_QUERY_TYPE_CLOSEST over OptixRay {o, tmin, d, tmax}, smallpt.cpp:395-403): rays = RAY_RANGE_DTYPE[n] or floats (n, 8); returns
        HIT_DTYPE[n].  The report of a sphere is its smaller root above max(tmin, 1e-4) if that is below min(tmax, 1e20)."""
        return _range_host(self, "trace_spheres_range", "spt_trace_spheres_range", rays)

    def trace_rays_range(self, rays):
        """The same against the current mesh scene (spt_trace_rays_range: triangles report max(tmin, 0) < t < min(tmax, 1e20))."""
        return _range_host(self, "trace_rays_range", "spt_trace_rays_range", rays)

    def trace_spheres_range_device(self, rays_t, hits_t=None, stream=None):
        """spt_trace_spheres_range_device: rays_t = contiguous float32 device tensor (n, 8); returns the float32 tensor (n, 11) of Hit records
        (hits_t if given), enqueued on `stream` (a torch stream; default: the current one)."""
        return _range_device(self, "trace_spheres_range_device", "spt_trace_spheres_range_device", rays_t, hits_t, stream)

    def trace_rays_range_device(self, rays_t, hits_t=None, stream=None):
        """spt_trace_rays_range_device: as trace_spheres_range_device, against the current mesh scene."""
        return _range_device(self, "trace_rays_range_device", "spt_trace_rays_range_device", rays_t, hits_t, stream)

    def last_query_path(self):
        """What the last trace_spheres* / trace_spheres_range* / occluded_spheres* query ran through and how many of its rays the walk handed to the exhaustive loop:
        ("exhaustive" | "grid" | "bvh" | None before the first query, fallback_rays).  Waits for that query."""
        fb = C.c_uint64(0)
        path = self._lib.spt_last_query_path(self._h, C.byref(fb))
        return {-1: None, 0: "exhaustive", 1: "grid", 2: "bvh"}[path], int(fb.value)

    def set_tuning(self, blocks_per_cu=0, variant=0):
        self._check(self._lib.spt_set_tuning(self._h, blocks_per_cu, variant))
        self._state["tuning"] = (int(blocks_per_cu), int(variant))
        self._state_version += 1

    def set_grid_pools(self, lane_owned=False, slots=0, ready=0, drain=0, min_batch=0, walk_iters=0):
        """Large sphere tables (csrc/spt_internal.h spt_set_grid_pools): keep the lane-owned grid kernel, or set the pool geometry of the
        default one (0 = default).  Results never depend on it."""
        self._check(self._lib.spt_set_grid_pools(self._h, int(lane_owned), slots, ready, drain, min_batch, walk_iters))   # (2: lane-owned with the tables in global memory, A/B)
        self._state["grid_pools"] = (bool(lane_owned), slots, ready, drain, min_batch, walk_iters)
        self._state_version += 1

    def render(self, w, h, samps_per_cell, seed=0, normalise=False, camera=None):
        """Full image to host memory: (h, w, 3) float32, row 0 = bottom.  Returns (image, stats)."""
        cam = camera if camera is not None else smallpt_camera(w, h)
        out = np.empty((h, w, 3), dtype=np.float32)
        st = SptStats()
        self._check(self._lib.spt_render(self._h, C.byref(cam), w, h, samps_per_cell, seed,
                                         FLAG_NORMALISE if normalise else 0,
                                         out.ctypes.data_as(C.c_void_p), C.byref(st)))
        return out, _stats_dict(st)

    def cpu_render_equivalent(self, w, h, spp, seed=0):
        """cpuRender(argv[1]=spp) semantics: samps = spp/4 (smallpt.cpp:276), normalised image."""
        return self.render(w, h, max(1, int(spp) // 4), seed=seed, normalise=True)

    def render_rows_device(self, out_tensor, w, h, row_begin, row_count, samps_per_cell, seed=0,
                           normalise=False, camera=None, stream=None):
        """Enqueues the render of rows [row_begin, row_begin+row_count) into ``out_tensor`` (a CUDA/HIP
        float32 torch tensor with row_count*w*3 elements on this context's device).  Asynchronous:
        call ``sync()`` for completion + statistics.  ``stream``: a raw hipStream_t handle (int), e.g.
        ``torch.cuda.current_stream().cuda_stream``; None = the context's own stream."""
        if out_tensor.numel() != row_count * w * 3 or not out_tensor.is_contiguous():
            raise ValueError("out_tensor must be contiguous with row_count*w*3 float32 elements")
        if str(out_tensor.dtype) != "torch.float32" or out_tensor.device.type != "cuda":
            raise ValueError("out_tensor must be a float32 tensor on the GPU")
        cam = camera if camera is not None else smallpt_camera(w, h)
        self._check(self._lib.spt_render_rows_device(
            self._h, C.byref(cam), w, h, row_begin, row_count, samps_per_cell, seed,
            FLAG_NORMALISE if normalise else 0, C.c_void_p(out_tensor.data_ptr()),
            C.c_void_p(stream) if stream else None))

    def render_aov(self, w, h, samps_per_cell, aov="normal", seed=0, normalise=False, camera=None):
        """First-hit feature buffer (spt_render_aov): 'normal', 'albedo', 'uv', 'dist' or 'emission' of the closest hit of every camera sample of
        ``render`` with the same arguments, folded in its order.  Returns ((h, w, 3) float32, stats)."""
        kind = _aov_kind(aov)
        cam = camera if camera is not None else smallpt_camera(w, h)
        out = np.empty((h, w, 3), dtype=np.float32)
        st = SptStats()
        self._check(self._lib.spt_render_aov(self._h, C.byref(cam), w, h, samps_per_cell, seed, kind,
                                             FLAG_NORMALISE if normalise else 0, out.ctypes.data_as(C.c_void_p), C.byref(st)))
        return out, _stats_dict(st)

    def render_aov_rows_device(self, out_tensor, w, h, row_begin, row_count, samps_per_cell, aov="normal", seed=0,
                               normalise=False, camera=None, stream=None):
        """Enqueues rows [row_begin, row_begin+row_count) of ``render_aov`` into ``out_tensor`` (as ``render_rows_device``).  Asynchronous:
        call ``sync()`` for completion + statistics."""
        kind = _aov_kind(aov)
        if out_tensor.numel() != row_count * w * 3 or not out_tensor.is_contiguous():
            raise ValueError("out_tensor must be contiguous with row_count*w*3 float32 elements")
        if str(out_tensor.dtype) != "torch.float32" or out_tensor.device.type != "cuda":
            raise ValueError("out_tensor must be a float32 tensor on the GPU")
        cam = camera if camera is not None else smallpt_camera(w, h)
        self._check(self._lib.spt_render_aov_rows_device(
            self._h, C.byref(cam), w, h, row_begin, row_count, samps_per_cell, seed, kind,
            FLAG_NORMALISE if normalise else 0, C.c_void_p(out_tensor.data_ptr()),
            C.c_void_p(stream) if stream else None))

    def render_aov_set(self, w, h, samps_per_cell, kinds=("normal", "albedo", "dist"), seed=0, normalise=False, camera=None):
        """Several first-hit feature buffers of the SAME samples from one launch (spt_render_aov_set): any of 'normal', 'albedo', 'uv',
        'dist' (as ``render_aov``), 'position' (the hit point) and 'coverage' (1 per hit: un-normalised, the pixel's hit count).
        Returns ({kind: (h, w, 3) float32}, stats)."""
        mask, names = _aov_set(kinds)
        cam = camera if camera is not None else smallpt_camera(w, h)
        outs = {k: np.empty((h, w, 3), dtype=np.float32) for k in names}
        ptrs = (C.c_void_p * len(names))(*[outs[k].ctypes.data for k in names])
        st = SptStats()
        self._check(self._lib.spt_render_aov_set(self._h, C.byref(cam), w, h, samps_per_cell, seed, mask,
                                                 FLAG_NORMALISE if normalise else 0, ptrs, C.byref(st)))
        return outs, _stats_dict(st)

    def render_aov_set_rows_device(self, out_tensors, w, h, row_begin, row_count, samps_per_cell, seed=0, normalise=False,
                                   camera=None, stream=None):
        """Enqueues rows [row_begin, row_begin+row_count) of ``render_aov_set`` into ``out_tensors`` = {kind: tensor} (each as
        ``render_aov_rows_device`` takes it).  Asynchronous: call ``sync()`` for completion + statistics."""
        if not isinstance(out_tensors, dict):
            raise ValueError("out_tensors must be a dict {kind: tensor}")
        mask, names = _aov_set(out_tensors.keys())
        for k in names:
            t = out_tensors[k]
            if t.numel() != row_count * w * 3 or not t.is_contiguous():
                raise ValueError(f"out_tensors[{k!r}] must be contiguous with row_count*w*3 float32 elements")
            if str(t.dtype) != "torch.float32" or t.device.type != "cuda":
                raise ValueError(f"out_tensors[{k!r}] must be a float32 tensor on the GPU")
        cam = camera if camera is not None else smallpt_camera(w, h)
        ptrs = (C.c_void_p * len(names))(*[out_tensors[k].data_ptr() for k in names])
        self._check(self._lib.spt_render_aov_set_rows_device(
            self._h, C.byref(cam), w, h, row_begin, row_count, samps_per_cell, seed, mask,
            FLAG_NORMALISE if normalise else 0, ptrs, C.c_void_p(stream) if stream else None))

    def denoise(self, beauty, normal, albedo, position, coverage, aov_samples, params=None):
        """Edge-avoiding wavelet filter (spt_denoise) of ``beauty`` guided by the four feature buffers: five (h, w, 3) float32 images,
        all UN-NORMALISED sums (``render(..., normalise=False)`` and ``render_aov_set(..., kinds=('normal', 'albedo', 'position',
        'coverage'))`` of the same camera, samples and seed); ``aov_samples`` = samples per pixel summed into the guides (4 * samps per
        launch).  Returns the filtered un-normalised sum, (h, w, 3) float32: divide by the sample count for display."""
        imgs = [np.ascontiguousarray(a, dtype=np.float32) for a in (beauty, normal, albedo, position, coverage)]
        if imgs[0].ndim != 3 or imgs[0].shape[2] != 3 or any(a.shape != imgs[0].shape for a in imgs):
            raise ValueError("denoise: five (h, w, 3) images of one size")
        h, w, _ = imgs[0].shape
        out = np.empty((h, w, 3), dtype=np.float32)
        p = _denoise_params(params)
        self._check(self._lib.spt_denoise(self._h, *[a.ctypes.data_as(C.c_void_p) for a in imgs], w, h, int(aov_samples), C.byref(p),
                                          out.ctypes.data_as(C.c_void_p)))
        return out

    def denoise_device(self, beauty_t, normal_t, albedo_t, position_t, coverage_t, out_t, w, h, aov_samples, params=None, stream=None):
        """The same on contiguous float32 CUDA tensors of w*h*3 elements (spt_denoise_device); asynchronous on ``stream`` (a raw
        hipStream_t, None = the context's stream).  ``out_t`` may not alias an input."""
        ts = (beauty_t, normal_t, albedo_t, position_t, coverage_t, out_t)
        for t in ts:
            if t.numel() != w * h * 3 or not t.is_contiguous() or str(t.dtype) != "torch.float32" or t.device.type != "cuda":
                raise ValueError("denoise_device: contiguous float32 tensors of w*h*3 elements on the GPU")
        p = _denoise_params(params)
        self._check(self._lib.spt_denoise_device(self._h, *[C.c_void_p(t.data_ptr()) for t in ts[:5]], w, h, int(aov_samples), C.byref(p),
                                                 C.c_void_p(out_t.data_ptr()), C.c_void_p(stream) if stream else None))

    def denoise_var(self, beauty, normal, albedo, position, coverage, m2, aov_samples, frames, params=None):
        """Variance-guided filter (spt_denoise_var): ``denoise`` with ``m2`` = (h, w) float32, the sum over ``frames`` >= 2 frames of the
        squared frame luminance (``progressive_begin(..., moments=True)`` / ``accumulate_moments_device``), ``beauty`` being the sum of
        the same frames.  Returns the filtered un-normalised sum, (h, w, 3) float32."""
        imgs = [np.ascontiguousarray(a, dtype=np.float32) for a in (beauty, normal, albedo, position, coverage)]
        m2 = np.ascontiguousarray(m2, dtype=np.float32)
        if imgs[0].ndim != 3 or imgs[0].shape[2] != 3 or any(a.shape != imgs[0].shape for a in imgs) or m2.shape != imgs[0].shape[:2]:
            raise ValueError("denoise_var: five (h, w, 3) images and one (h, w) image of one size")
        h, w, _ = imgs[0].shape
        out = np.empty((h, w, 3), dtype=np.float32)
        p = _denoise_var_params(params)
        self._check(self._lib.spt_denoise_var(self._h, *[a.ctypes.data_as(C.c_void_p) for a in imgs], m2.ctypes.data_as(C.c_void_p), w, h,
                                              int(aov_samples), int(frames), C.byref(p), out.ctypes.data_as(C.c_void_p)))
        return out

    def denoise_var_device(self, beauty_t, normal_t, albedo_t, position_t, coverage_t, m2_t, out_t, w, h, aov_samples, frames, params=None,
                           stream=None):
        """The same on contiguous float32 CUDA tensors (spt_denoise_var_device): w*h*3 elements each, ``m2_t`` w*h; asynchronous on
        ``stream`` (a raw hipStream_t, None = the context's stream).  ``out_t`` may not alias an input."""
        ts = (beauty_t, normal_t, albedo_t, position_t, coverage_t, out_t, m2_t)
        for t, n in zip(ts, (w * h * 3,) * 6 + (w * h,)):
            if t.numel() != n or not t.is_contiguous() or str(t.dtype) != "torch.float32" or t.device.type != "cuda":
                raise ValueError("denoise_var_device: contiguous float32 tensors of w*h*3 (m2_t: w*h) elements on the GPU")
        p = _denoise_var_params(params)
        self._check(self._lib.spt_denoise_var_device(self._h, *[C.c_void_p(t.data_ptr()) for t in ts[:5]], C.c_void_p(m2_t.data_ptr()), w, h,
                                                     int(aov_samples), int(frames), C.byref(p), C.c_void_p(out_t.data_ptr()),
                                                     C.c_void_p(stream) if stream else None))

    def display(self, rgb_sum, params=None):
        """8-bit display transform on the device (spt_display): q = toInt(rgb_sum * weight) per channel of an (h, w, 3) float32 image
        (row 0 = bottom), bit-exact to toInt (NaN -> 0).  Returns uint8 (h, w, 3) or (h, w, 4) per ``params`` (a ``DisplayParams``)."""
        img = np.ascontiguousarray(rgb_sum, dtype=np.float32)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("display: one (h, w, 3) image")
        h, w, _ = img.shape
        dp = _display_params(params)
        out = np.empty((h, w, dp.channels), dtype=np.uint8)
        p = dp.as_c()
        self._check(self._lib.spt_display(self._h, img.ctypes.data_as(C.c_void_p), w, h, C.byref(p), out.ctypes.data_as(C.c_void_p)))
        return out

    def display_device(self, rgb_sum_t, w, h, params=None, out_t=None, stream=None):
        """The same on a float32 CUDA tensor of w*h*3 elements (spt_display_device); asynchronous on ``stream`` (a raw hipStream_t, None =
        the context's stream).  ``out_t``: a contiguous uint8 CUDA tensor of w*h*(3|4) elements (any alignment), allocated when None.
        Returns ``out_t`` viewed as (h, w, 3|4)."""
        dp = _display_params(params)
        if rgb_sum_t.numel() != w * h * 3 or not rgb_sum_t.is_contiguous() or str(rgb_sum_t.dtype) != "torch.float32" or rgb_sum_t.device.type != "cuda":
            raise ValueError("display_device: a contiguous float32 tensor of w*h*3 elements on the GPU")
        if out_t is None:
            import torch
            out_t = torch.empty(w * h * dp.channels, dtype=torch.uint8, device=rgb_sum_t.device)
        if out_t.numel() != w * h * dp.channels or not out_t.is_contiguous() or str(out_t.dtype) != "torch.uint8" or out_t.device.type != "cuda":
            raise ValueError("display_device: out_t is a contiguous uint8 tensor of w*h*(3|4) elements on the GPU")
        p = dp.as_c()
        self._check(self._lib.spt_display_device(self._h, C.c_void_p(rgb_sum_t.data_ptr()), w, h, C.byref(p), C.c_void_p(out_t.data_ptr()),
                                                 C.c_void_p(stream) if stream else None))
        return out_t.view(h, w, dp.channels)

    def temporal_accumulate(self, frame, normal, position, coverage, frame_samples, camera, prev_camera=None, history=None, params=None,
                            want=("rgb", "var", "len")):
        """One step of the temporal accumulation (spt_temporal_accumulate): ``frame`` the un-normalised beauty sum and ``normal``,
        ``position``, ``coverage`` the feature sums of the same camera, samples and seed, (h, w, 3) float32 each; ``frame_samples`` = 4 *
        samps; ``history`` the (3, h, w, 4) float32 array a previous step returned (None: no history) and ``prev_camera`` the camera of
        that step.  Returns (history', {'rgb': (h, w, 3) mean, 'var': (h, w), 'len': (h, w)}) with the outputs named in ``want``."""
        imgs = [np.ascontiguousarray(a, dtype=np.float32) for a in (frame, normal, position, coverage)]
        if imgs[0].ndim != 3 or imgs[0].shape[2] != 3 or any(a.shape != imgs[0].shape for a in imgs):
            raise ValueError("temporal_accumulate: four (h, w, 3) images of one size")
        h, w, _ = imgs[0].shape
        if history is not None:
            history = np.ascontiguousarray(history, dtype=np.float32)
            if history.shape != (3, h, w, 4):
                raise ValueError("temporal_accumulate: history is a (3, h, w, 4) float32 array")
            if prev_camera is None:
                raise ValueError("temporal_accumulate: a history needs the camera it was written with")
        unknown = set(want) - {"rgb", "var", "len"}
        if unknown:
            raise ValueError(f"temporal_accumulate: unknown outputs {sorted(unknown)}")
        nxt = np.empty((3, h, w, 4), dtype=np.float32)
        outs = {k: np.empty((h, w, 3) if k == "rgb" else (h, w), dtype=np.float32) for k in ("rgb", "var", "len") if k in want}
        ptr = lambda k: outs[k].ctypes.data_as(C.c_void_p) if k in outs else None       # noqa: E731
        p = _temporal_params(params)
        self._check(self._lib.spt_temporal_accumulate(
            self._h, *[a.ctypes.data_as(C.c_void_p) for a in imgs], w, h, int(frame_samples), C.byref(camera),
            C.byref(prev_camera) if prev_camera is not None else None, history.ctypes.data_as(C.c_void_p) if history is not None else None,
            nxt.ctypes.data_as(C.c_void_p), C.byref(p), ptr("rgb"), ptr("var"), ptr("len")))
        return nxt, outs

    def temporal_accumulate_device(self, frame_t, normal_t, position_t, coverage_t, w, h, frame_samples, camera, hist_next_t, prev_camera=None,
                                   hist_prev_t=None, params=None, out_rgb_t=None, out_var_t=None, out_len_t=None, stream=None):
        """The same on float32 CUDA tensors (spt_temporal_accumulate_device): the four images w*h*3 elements, the histories w*h*12 elements
        and 16-byte aligned, ``out_rgb_t`` w*h*3 and ``out_var_t`` / ``out_len_t`` w*h elements or None.  Asynchronous on ``stream`` (a raw
        hipStream_t, None = the context's stream).  No output may overlap an input."""
        sizes = [(frame_t, w * h * 3), (normal_t, w * h * 3), (position_t, w * h * 3), (coverage_t, w * h * 3), (hist_next_t, w * h * 12),
                 (hist_prev_t, w * h * 12), (out_rgb_t, w * h * 3), (out_var_t, w * h), (out_len_t, w * h)]
        for t, n in sizes:
            if t is not None and (t.numel() != n or not t.is_contiguous() or str(t.dtype) != "torch.float32" or t.device.type != "cuda"):
                raise ValueError("temporal_accumulate_device: contiguous float32 tensors on the GPU of w*h*3 (images), w*h*12 (histories) and w*h elements")
        if hist_prev_t is not None and prev_camera is None:
            raise ValueError("temporal_accumulate_device: a history needs the camera it was written with")
        dp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None            # noqa: E731
        p = _temporal_params(params)
        self._check(self._lib.spt_temporal_accumulate_device(
            self._h, dp(frame_t), dp(normal_t), dp(position_t), dp(coverage_t), w, h, int(frame_samples), C.byref(camera),
            C.byref(prev_camera) if prev_camera is not None else None, dp(hist_prev_t), dp(hist_next_t), C.byref(p), dp(out_rgb_t), dp(out_var_t),
            dp(out_len_t), C.c_void_p(stream) if stream else None))

    def temporal_variance(self, history, params=None, var=False):
        """SVGF's variance estimate from a temporal history (spt_temporal_variance): ``history`` the (3, h, w, 4) float32 array
        ``temporal_accumulate`` returns.  A pixel whose history length is at least ``params.min_len`` takes its temporal variance, a
        younger one the boosted 7 x 7 spatial estimate.  Returns the (h, w) float32 variance of the pixel's MEAN (what ``denoise_pvar``
        takes); with ``var`` a tuple (that, the (h, w) estimate of one frame's variance)."""
        history = np.ascontiguousarray(history, dtype=np.float32)
        if history.ndim != 4 or history.shape[0] != 3 or history.shape[3] != 4:
            raise ValueError("temporal_variance: history is a (3, h, w, 4) float32 array")
        _, h, w, _ = history.shape
        vm = np.empty((h, w), dtype=np.float32)
        v = np.empty((h, w), dtype=np.float32) if var else None
        p = _temporal_var_params(params)
        self._check(self._lib.spt_temporal_variance(self._h, history.ctypes.data_as(C.c_void_p), w, h, C.byref(p), vm.ctypes.data_as(C.c_void_p),
                                                    v.ctypes.data_as(C.c_void_p) if var else None))
        return (vm, v) if var else vm

    def temporal_variance_device(self, hist_t, w, h, out_var_mean_t, out_var_t=None, params=None, stream=None):
        """The same on float32 CUDA tensors (spt_temporal_variance_device): ``hist_t`` w*h*12 elements and 16-byte aligned, the outputs w*h
        elements (``out_var_t`` or None).  Asynchronous on ``stream`` (a raw hipStream_t, None = the context's stream).  No output may
        overlap the history or the other output."""
        for t, n in ((hist_t, w * h * 12), (out_var_mean_t, w * h), (out_var_t, w * h)):
            if t is not None and (t.numel() != n or not t.is_contiguous() or str(t.dtype) != "torch.float32" or t.device.type != "cuda"):
                raise ValueError("temporal_variance_device: contiguous float32 tensors on the GPU of w*h*12 (history) and w*h elements")
        p = _temporal_var_params(params)
        self._check(self._lib.spt_temporal_variance_device(self._h, C.c_void_p(hist_t.data_ptr()), w, h, C.byref(p), C.c_void_p(out_var_mean_t.data_ptr()),
                                                           C.c_void_p(out_var_t.data_ptr()) if out_var_t is not None else None,
                                                           C.c_void_p(stream) if stream else None))

    def _demod_host(self, who, fn, colour, albedo, coverage, emission, counts, params):
        imgs = [np.ascontiguousarray(a, dtype=np.float32) for a in (colour, albedo, coverage) + ((emission,) if emission is not None else ())]
        if imgs[0].ndim != 3 or imgs[0].shape[2] != 3 or any(a.shape != imgs[0].shape for a in imgs):
            raise ValueError(f"{who}: (h, w, 3) images of one size")
        h, w, _ = imgs[0].shape
        out = np.empty((h, w, 3), dtype=np.float32)
        p = _demod_params(params)
        ptr = [a.ctypes.data_as(C.c_void_p) for a in imgs] + ([None] if emission is None else [])
        self._check(getattr(self._lib, fn)(self._h, *ptr, w, h, *[int(n) for n in counts], C.byref(p), out.ctypes.data_as(C.c_void_p)))
        return out

    def demodulate(self, beauty, albedo, coverage, emission, beauty_samples, aov_samples, params=None):
        """Colour to illumination (spt_demodulate): ``beauty`` the un-normalised (h, w, 3) sum over ``beauty_samples`` samples per pixel,
        ``albedo`` / ``coverage`` / ``emission`` (or None) the un-normalised sums over ``aov_samples`` as ``render_aov_set`` and
        ``render_aov(aov='emission')`` return them.  Returns the (h, w, 3) float32 MEAN illumination: what the filters take as their
        beauty."""
        return self._demod_host("demodulate", "spt_demodulate", beauty, albedo, coverage, emission, (beauty_samples, aov_samples), params)

    def remodulate(self, illum, albedo, coverage, emission, aov_samples, params=None):
        """The way back (spt_remodulate): the (filtered) mean illumination times the albedo plus the unmodulated part; returns the
        (h, w, 3) float32 mean colour (``display`` takes it with weight 1)."""
        return self._demod_host("remodulate", "spt_remodulate", illum, albedo, coverage, emission, (aov_samples,), params)

    def _demod_device(self, who, fn, colour_t, albedo_t, coverage_t, emission_t, out_t, w, h, counts, params, stream):
        for t in (colour_t, albedo_t, coverage_t, emission_t, out_t):
            if t is not None and (t.numel() != w * h * 3 or not t.is_contiguous() or str(t.dtype) != "torch.float32" or t.device.type != "cuda"):
                raise ValueError(f"{who}: contiguous float32 tensors on the GPU of w*h*3 elements")
        if colour_t is None or albedo_t is None or coverage_t is None or out_t is None:
            raise ValueError(f"{who}: only the emission may be None")
        p = _demod_params(params)
        self._check(getattr(self._lib, fn)(self._h, C.c_void_p(colour_t.data_ptr()), C.c_void_p(albedo_t.data_ptr()), C.c_void_p(coverage_t.data_ptr()),
                       C.c_void_p(emission_t.data_ptr()) if emission_t is not None else None, w, h, *[int(n) for n in counts], C.byref(p),
                       C.c_void_p(out_t.data_ptr()), C.c_void_p(stream) if stream else None))

    def demodulate_device(self, beauty_t, albedo_t, coverage_t, emission_t, out_t, w, h, beauty_samples, aov_samples, params=None, stream=None):
        """``demodulate`` on float32 CUDA tensors of w*h*3 elements (spt_demodulate_device), asynchronous on ``stream`` (a raw hipStream_t,
        None = the context's stream).  ``out_t`` may be ``beauty_t`` itself; it may overlap nothing else."""
        self._demod_device("demodulate_device", "spt_demodulate_device", beauty_t, albedo_t, coverage_t, emission_t, out_t, w, h,
                           (beauty_samples, aov_samples), params, stream)

    def remodulate_device(self, illum_t, albedo_t, coverage_t, emission_t, out_t, w, h, aov_samples, params=None, stream=None):
        """``remodulate`` on float32 CUDA tensors (spt_remodulate_device); ``out_t`` may be ``illum_t`` itself."""
        self._demod_device("remodulate_device", "spt_remodulate_device", illum_t, albedo_t, coverage_t, emission_t, out_t, w, h,
                           (aov_samples,), params, stream)

    # ---- the wavefront seam (spt_wavefront_*): camera paths, one shadePaths step, accumulation ----
    @staticmethod
    def wavefront_path_count(w, row_count, samps_per_cell):
        """spt_wavefront_path_count: the camera paths of a band, 4 * w * row_count * samps."""
        return int(load_library().spt_wavefront_path_count(int(w), int(row_count), int(samps_per_cell)))

    def _wf_window(self, w, h, samps, row_begin, row_count, first, count):
        row_count = h - row_begin if row_count is None else row_count
        if count is None:
            count = max(0, self.wavefront_path_count(w, row_count, samps) - first)
        return int(row_count), int(count)

    def wavefront_generate(self, w, h, samps_per_cell, seed=0, camera=None, row_begin=0, row_count=None, first=0, count=None):
        """Camera paths first .. first + count of a band (spt_wavefront_generate), in the order ((local pixel * 4 + cell) * samps + s): the
        rays and keys ``render`` traces for the same arguments.  Returns (RAY_DTYPE[count], PATH_DTYPE[count])."""
        cam = camera if camera is not None else smallpt_camera(w, h)
        row_count, count = self._wf_window(w, h, samps_per_cell, row_begin, row_count, first, count)
        rays, paths = np.zeros(count, dtype=RAY_DTYPE), np.zeros(count, dtype=PATH_DTYPE)
        self._check(self._lib.spt_wavefront_generate(self._h, C.byref(cam), w, h, row_begin, row_count, samps_per_cell, seed, first, count,
                                                     rays.ctypes.data_as(C.c_void_p), paths.ctypes.data_as(C.c_void_p)))
        return rays, paths

    def wavefront_generate_device(self, rays_t, paths_t, w, h, samps_per_cell, seed=0, camera=None, row_begin=0, row_count=None, first=0,
                                  count=None, stream=None):
        """The same into device tensors (spt_wavefront_generate_device): ``rays_t`` float32 (>= count, 6), ``paths_t`` int32 (>= count, 12),
        16-byte aligned (a path is 12 words, PATH_DTYPE).  Asynchronous on ``stream`` (a raw hipStream_t, None = the context's stream)."""
        cam = camera if camera is not None else smallpt_camera(w, h)
        row_count, count = self._wf_window(w, h, samps_per_cell, row_begin, row_count, first, count)
        _wf_tensor("wavefront_generate_device", rays_t, "torch.float32", count, 6)
        _wf_tensor("wavefront_generate_device", paths_t, "torch.int32", count, 12)
        self._check(self._lib.spt_wavefront_generate_device(self._h, C.byref(cam), w, h, row_begin, row_count, samps_per_cell, seed, first, count,
                                                            C.c_void_p(rays_t.data_ptr()), C.c_void_p(paths_t.data_ptr()),
                                                            C.c_void_p(stream) if stream else None))
        return count

    def wavefront_shade(self, rays, paths, hits):
        """One shadePaths step (spt_wavefront_shade) over RAY_DTYPE / PATH_DTYPE / HIT_DTYPE arrays of one length, with the current scene's
        materials and environment.  Returns (events (n, 3) float32, next rays, next paths, depth-cap kills): the children in the order of
        the reference's nextPaths -- ascending parent, reflected before transmitted."""
        rays = _ray_array(rays)
        paths, hits = np.ascontiguousarray(paths, dtype=PATH_DTYPE), np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        n = len(rays)
        if paths.shape != (n,) or hits.shape != (n,):
            raise ValueError("wavefront_shade: rays, paths and hits of one length")
        events = np.zeros((n, 3), dtype=np.float32)
        nrays, npaths = np.zeros(2 * n, dtype=RAY_DTYPE), np.zeros(2 * n, dtype=PATH_DTYPE)
        counts = (C.c_uint64 * 2)()
        self._check(self._lib.spt_wavefront_shade(self._h, rays.ctypes.data_as(C.c_void_p), paths.ctypes.data_as(C.c_void_p),
                                                  hits.ctypes.data_as(C.c_void_p), n, nrays.ctypes.data_as(C.c_void_p),
                                                  npaths.ctypes.data_as(C.c_void_p), 2 * n, events.ctypes.data_as(C.c_void_p), counts))
        m = int(counts[0])
        return events, nrays[:m].copy(), npaths[:m].copy(), int(counts[1])

    def wavefront_shade_device(self, rays_t, paths_t, hits_t, next_rays_t, next_paths_t, events_t, counts_t, n=None, stream=None):
        """The same on device tensors (spt_wavefront_shade_device): float32 rays (>= n, 6), hits (>= n, 11) and events (>= n, 3), int32
        paths (>= n, 12), the outputs ``next_rays_t`` / ``next_paths_t`` with room for 2 n children, ``counts_t`` int64 (2,) =
        {children, depth-cap kills}.  n = None: the rays' length.  Asynchronous on ``stream`` (a raw hipStream_t, None = the context's)."""
        who = "wavefront_shade_device"
        n = int(rays_t.shape[0] if n is None else n)
        _wf_tensor(who, rays_t, "torch.float32", n, 6)
        _wf_tensor(who, paths_t, "torch.int32", n, 12)
        _wf_tensor(who, hits_t, "torch.float32", n, 11)
        _wf_tensor(who, events_t, "torch.float32", n, 3)
        _wf_tensor(who, next_rays_t, "torch.float32", 0, 6)
        _wf_tensor(who, next_paths_t, "torch.int32", 0, 12)
        if str(counts_t.dtype) != "torch.int64" or counts_t.numel() != 2 or counts_t.device.type != "cuda":
            raise ValueError(f"{who}: counts_t is an int64 device tensor of 2 elements")
        cap = min(int(next_rays_t.shape[0]), int(next_paths_t.shape[0]))
        self._check(self._lib.spt_wavefront_shade_device(self._h, C.c_void_p(rays_t.data_ptr()), C.c_void_p(paths_t.data_ptr()), C.c_void_p(hits_t.data_ptr()),
                                                         n, C.c_void_p(next_rays_t.data_ptr()), C.c_void_p(next_paths_t.data_ptr()), cap,
                                                         C.c_void_p(events_t.data_ptr()), C.c_void_p(counts_t.data_ptr()),
                                                         C.c_void_p(stream) if stream else None))

    def wavefront_accumulate(self, paths, events, image, pixel_first=0):
        """image[p - pixel_first] += the events of the paths of pixel p, in order (spt_wavefront_accumulate): ``image`` (pixels, 3) float32 (any
        shape of 3 * pixels elements); returns the new image, same shape.  The paths of one pixel must form one run of the array."""
        paths = np.ascontiguousarray(paths, dtype=PATH_DTYPE)
        events = np.ascontiguousarray(events, dtype=np.float32).reshape(-1, 3)
        out = np.array(image, dtype=np.float32, order="C")
        if len(events) != len(paths) or out.size % 3:
            raise ValueError("wavefront_accumulate: one event per path, an image of float3 pixels")
        self._check(self._lib.spt_wavefront_accumulate(self._h, paths.ctypes.data_as(C.c_void_p), events.ctypes.data_as(C.c_void_p), len(paths),
                                                       int(pixel_first), out.size // 3, out.ctypes.data_as(C.c_void_p)))
        return out

    def wavefront_accumulate_device(self, paths_t, events_t, image_t, n=None, pixel_first=0, stream=None):
        """The same on device tensors (spt_wavefront_accumulate_device): ``image_t`` float32 of 3 * pixels elements, updated in place."""
        who = "wavefront_accumulate_device"
        n = int(paths_t.shape[0] if n is None else n)
        _wf_tensor(who, paths_t, "torch.int32", n, 12)
        _wf_tensor(who, events_t, "torch.float32", n, 3)
        if str(image_t.dtype) != "torch.float32" or image_t.device.type != "cuda" or not image_t.is_contiguous() or image_t.numel() % 3:
            raise ValueError(f"{who}: image_t is a contiguous float32 device tensor of float3 pixels")
        self._check(self._lib.spt_wavefront_accumulate_device(self._h, C.c_void_p(paths_t.data_ptr()), C.c_void_p(events_t.data_ptr()), n, int(pixel_first),
                                                              image_t.numel() // 3, C.c_void_p(image_t.data_ptr()), C.c_void_p(stream) if stream else None))

    def wavefront_render(self, w, h, samps_per_cell, seed=0, normalise=False, camera=None):
        """Renderer::render's loop behind the boundary (spt_wavefront_render): generate, the scene's closest-hit query, shade, accumulate,
        until no path is left.  Returns ((h, w, 3) float32, stats) -- the stats of ``render``; the image adds a pixel's events bounce by
        bounce, so it equals ``wavefront_loop``'s bit for bit and ``render``'s up to the order of the float32 additions."""
        cam = camera if camera is not None else smallpt_camera(w, h)
        out = np.empty((h, w, 3), dtype=np.float32)
        st = SptStats()
        self._check(self._lib.spt_wavefront_render(self._h, C.byref(cam), w, h, samps_per_cell, seed, FLAG_NORMALISE if normalise else 0,
                                                   out.ctypes.data_as(C.c_void_p), C.byref(st)))
        return out, _stats_dict(st)

    def set_wavefront_chunk(self, pixels=0):
        """Pixels per chunk of ``wavefront_render`` (csrc/spt_internal.h; 0 = the default).  Results never depend on it."""
        self._check(self._lib.spt_set_wavefront_chunk(self._h, int(pixels)))

    def wavefront_loop(self, w, h, samps_per_cell, seed=0, camera=None, keep=False, stream=None):
        """The loop ``wavefront_render`` runs, driven from outside: ``wavefront_generate_device``, then per bounce the scene's closest-hit
        query (spt_trace_spheres_device or spt_trace_rays_device), ``wavefront_shade_device`` and ``wavefront_accumulate_device`` over torch
        tensors, until no child is left.  ``stream``: a raw hipStream_t for every step (None = the context's stream).  Returns
        (image (h, w, 3) float32 un-normalised, {"samples", "bounces", "max_depth_kills"}), and with ``keep`` a third value: the list of
        (PATH_DTYPE paths, (n, 3) events, HIT_DTYPE hits) of every iteration."""
        import torch
        cam = camera if camera is not None else smallpt_camera(w, h)
        dev = torch.device("cuda", self.device_id)
        n = self.wavefront_path_count(w, h, samps_per_cell)
        f32 = lambda rows, cols: torch.empty((max(1, rows), cols), dtype=torch.float32, device=dev)
        i32 = lambda rows: torch.empty((max(1, rows), 12), dtype=torch.int32, device=dev)
        rays, paths = f32(n, 6), i32(n)
        image = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)                          # torch's fills are done before another stream writes the tensors
        sp = C.c_void_p(stream) if stream else None
        trace = self._lib.spt_trace_spheres_device if self._state["scene"][0] == "spheres" else self._lib.spt_trace_rays_device
        self.wavefront_generate_device(rays, paths, w, h, samps_per_cell, seed=seed, camera=cam, stream=stream)
        stats = {"samples": n, "bounces": 0, "max_depth_kills": 0}
        kept = []
        while n:
            hits, events, nrays, npaths = f32(n, 11), f32(n, 3), f32(2 * n, 6), i32(2 * n)
            torch.cuda.synchronize(dev)
            self._check(trace(self._h, C.c_void_p(rays.data_ptr()), n, C.c_void_p(hits.data_ptr()), sp))
            self.wavefront_shade_device(rays, paths, hits, nrays, npaths, events, counts, n=n, stream=stream)
            self.wavefront_accumulate_device(paths, events, image, n=n, stream=stream)
            torch.cuda.synchronize(dev)
            if keep:
                kept.append((paths[:n].cpu().numpy().view(PATH_DTYPE).reshape(-1), events[:n].cpu().numpy(),
                             hits[:n].cpu().numpy().view(HIT_DTYPE).reshape(-1)))
            children, kills = (int(v) for v in counts.cpu())
            stats["bounces"] += n
            stats["max_depth_kills"] += kills
            rays, paths, n = nrays, npaths, children
        out = image.cpu().numpy()
        return (out, stats, kept) if keep else (out, stats)

    def denoise_pvar(self, beauty, normal, albedo, position, coverage, variance, aov_samples, params=None):
        """Variance-guided filter with a caller's per-pixel variance (spt_denoise_pvar): ``denoise_var`` with ``variance`` = (h, w)
        float32, >= 0, the variance of the luminance of ``beauty`` as given (a sum or a mean) in place of ``m2`` and ``frames``.
        Returns the filtered image, (h, w, 3) float32."""
        imgs = [np.ascontiguousarray(a, dtype=np.float32) for a in (beauty, normal, albedo, position, coverage)]
        variance = np.ascontiguousarray(variance, dtype=np.float32)
        if imgs[0].ndim != 3 or imgs[0].shape[2] != 3 or any(a.shape != imgs[0].shape for a in imgs) or variance.shape != imgs[0].shape[:2]:
            raise ValueError("denoise_pvar: five (h, w, 3) images and one (h, w) image of one size")
        h, w, _ = imgs[0].shape
        out = np.empty((h, w, 3), dtype=np.float32)
        p = _denoise_var_params(params)
        self._check(self._lib.spt_denoise_pvar(self._h, *[a.ctypes.data_as(C.c_void_p) for a in imgs], variance.ctypes.data_as(C.c_void_p), w, h,
                                               int(aov_samples), C.byref(p), out.ctypes.data_as(C.c_void_p)))
        return out

    def denoise_pvar_device(self, beauty_t, normal_t, albedo_t, position_t, coverage_t, variance_t, out_t, w, h, aov_samples, params=None, stream=None):
        """The same on contiguous float32 CUDA tensors (spt_denoise_pvar_device): w*h*3 elements each, ``variance_t`` w*h; asynchronous on
        ``stream`` (a raw hipStream_t, None = the context's stream).  ``out_t`` may not alias an input."""
        ts = (beauty_t, normal_t, albedo_t, position_t, coverage_t, out_t, variance_t)
        for t, n in zip(ts, (w * h * 3,) * 6 + (w * h,)):
            if t.numel() != n or not t.is_contiguous() or str(t.dtype) != "torch.float32" or t.device.type != "cuda":
                raise ValueError("denoise_pvar_device: contiguous float32 tensors of w*h*3 (variance_t: w*h) elements on the GPU")
        p = _denoise_var_params(params)
        self._check(self._lib.spt_denoise_pvar_device(self._h, *[C.c_void_p(t.data_ptr()) for t in ts[:5]], C.c_void_p(variance_t.data_ptr()), w, h,
                                                      int(aov_samples), C.byref(p), C.c_void_p(out_t.data_ptr()), C.c_void_p(stream) if stream else None))

    def accumulate_moments_device(self, accum_t, m2_t, frame_t, clear=False, stream=None):
        """accum (``clear``: =, else +=) frame and m2 (=, +=) the squared luminance of frame, one kernel (spt_accumulate_moments_device):
        contiguous float32 CUDA tensors, ``accum_t`` and ``frame_t`` of npix*3 elements and 16-byte aligned, ``m2_t`` of npix elements.
        Asynchronous on ``stream`` (a raw hipStream_t, None = the context's stream)."""
        npix = m2_t.numel()
        for t, n in ((accum_t, npix * 3), (frame_t, npix * 3), (m2_t, npix)):
            if t.numel() != n or not t.is_contiguous() or str(t.dtype) != "torch.float32" or t.device.type != "cuda":
                raise ValueError("accumulate_moments_device: contiguous float32 tensors of npix*3, npix and npix*3 elements on the GPU")
        self._check(self._lib.spt_accumulate_moments_device(self._h, C.c_void_p(accum_t.data_ptr()), C.c_void_p(m2_t.data_ptr()),
                                                            C.c_void_p(frame_t.data_ptr()), npix, 1 if clear else 0,
                                                            C.c_void_p(stream) if stream else None))

    # The render thread's loop behind the C-ABI (spt_progressive_*): radiance and feature accumulators resident on the device.
    def progressive_begin(self, w, h, aov_kinds=None, moments=False):
        """spt_progressive_begin, spt_progressive_aov_begin for ``aov_kinds`` (names as ``render_aov_set``) when given, and
        spt_progressive_moments_begin when ``moments``: the loop then also sums the frames' squared luminance per pixel."""
        self._check(self._lib.spt_progressive_begin(self._h, w, h))
        self._prog = (w, h, ())
        if aov_kinds is not None:
            mask, names = _aov_set(aov_kinds)
            self._check(self._lib.spt_progressive_aov_begin(self._h, mask))
            self._prog = (w, h, tuple(names))
        if moments:
            self._check(self._lib.spt_progressive_moments_begin(self._h))

    def progressive_frame(self, samps_per_cell, seed, clear=False, camera=None):
        """One radiance frame added to (``clear``: replacing) accumBuffer; blocking.  Returns the stats."""
        w, h, _ = self._prog_size("progressive_frame")
        cam = camera if camera is not None else smallpt_camera(w, h)
        st = SptStats()
        self._check(self._lib.spt_progressive_frame(self._h, C.byref(cam), samps_per_cell, seed, 1 if clear else 0, C.byref(st)))
        return _stats_dict(st)

    def progressive_aov_frame(self, samps_per_cell, seed, clear=False, camera=None):
        """One fused launch of the selected feature buffers added to (``clear``: replacing) their accumulators; blocking."""
        w, h, _ = self._prog_size("progressive_aov_frame")
        cam = camera if camera is not None else smallpt_camera(w, h)
        st = SptStats()
        self._check(self._lib.spt_progressive_aov_frame(self._h, C.byref(cam), samps_per_cell, seed, 1 if clear else 0, C.byref(st)))
        return _stats_dict(st)

    def progressive_snapshot(self, kind=None):
        """accumBuffer (kind None) or the accumulator of one selected feature kind: (h, w, 3) float32, un-normalised."""
        w, h, _ = self._prog_size("progressive_snapshot")
        out = np.empty((h, w, 3), dtype=np.float32)
        if kind is None:
            self._check(self._lib.spt_progressive_snapshot(self._h, out.ctypes.data_as(C.c_void_p)))
        else:
            self._check(self._lib.spt_progressive_aov_snapshot(self._h, 1 << AOV_SET_KINDS[kind], out.ctypes.data_as(C.c_void_p)))
        return out

    def progressive_denoised_snapshot(self, aov_samples, params=None):
        """accumBuffer filtered under the feature accumulators (spt_progressive_denoised_snapshot): needs ``progressive_begin`` with at
        least normal, albedo, position and coverage.  ``aov_samples`` = frames * 4 * samps accumulated into the features.  Returns the
        filtered un-normalised sum, (h, w, 3) float32; neither accumulator changes."""
        w, h, _ = self._prog_size("progressive_denoised_snapshot")
        out = np.empty((h, w, 3), dtype=np.float32)
        p = _denoise_params(params)
        self._check(self._lib.spt_progressive_denoised_snapshot(self._h, int(aov_samples), C.byref(p), out.ctypes.data_as(C.c_void_p)))
        return out

    def progressive_variance_snapshot(self):
        """((h, w) float32, frames): the biased variance estimate of one frame's luminance per pixel and the frames accumulated since the
        last clearing frame (spt_progressive_variance_snapshot); needs ``progressive_begin(..., moments=True)`` and a clearing frame."""
        w, h, _ = self._prog_size("progressive_variance_snapshot")
        out = np.empty((h, w), dtype=np.float32)
        n = C.c_uint32(0)
        self._check(self._lib.spt_progressive_variance_snapshot(self._h, out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out, int(n.value)

    def progressive_denoised_var_snapshot(self, aov_samples, params=None):
        """accumBuffer under the variance-guided filter (spt_progressive_denoised_var_snapshot): ``progressive_denoised_snapshot`` with
        the loop's second moments; needs ``moments=True``, a clearing frame and at least two frames since."""
        w, h, _ = self._prog_size("progressive_denoised_var_snapshot")
        out = np.empty((h, w, 3), dtype=np.float32)
        p = _denoise_var_params(params)
        self._check(self._lib.spt_progressive_denoised_var_snapshot(self._h, int(aov_samples), C.byref(p), out.ctypes.data_as(C.c_void_p)))
        return out

    def progressive_display_snapshot(self, params=None, source="accum", aov_samples=0, filter_params=None):
        """The loop's picture as 8-bit colour straight from the device (spt_progressive_display_snapshot): ``source`` 'accum' (accumBuffer),
        'denoised' (``filter_params`` a ``DenoiseParams`` or None) or 'denoised_var' (a ``DenoiseVarParams`` or None), the filters with
        ``aov_samples`` as in ``progressive_denoised_snapshot``; then ``display`` with ``params`` -- the caller puts the weight
        1/(frames * spp) there.  Only w*h*(3|4) bytes cross the host link.  Returns uint8 (h, w, 3|4); nothing of the loop changes."""
        w, h, _ = self._prog_size("progressive_display_snapshot")
        dp = _display_params(params)
        out = np.empty((h, w, dp.channels), dtype=np.uint8)
        p = dp.as_c()
        src = {"accum": DISPLAY_SRC_ACCUM, "denoised": DISPLAY_SRC_DENOISED, "denoised_var": DISPLAY_SRC_DENOISED_VAR}.get(source, source)
        fp = None
        if src == DISPLAY_SRC_DENOISED:
            fp = _denoise_params(filter_params)
        elif src == DISPLAY_SRC_DENOISED_VAR:
            fp = _denoise_var_params(filter_params)
        elif filter_params is not None:
            raise ValueError("progressive_display_snapshot: source 'accum' takes no filter_params")
        self._check(self._lib.spt_progressive_display_snapshot(self._h, int(src), int(aov_samples), C.byref(fp) if fp is not None else None, C.byref(p),
                                                               out.ctypes.data_as(C.c_void_p)))
        return out

    def progressive_temporal_begin(self, params=None):
        """spt_progressive_temporal_begin after ``progressive_begin``: a second loop over normalised means with a per-pixel history
        length, which keeps its history across camera moves (``params`` a ``TemporalParams``)."""
        self._prog_size("progressive_temporal_begin")
        p = _temporal_params(params)
        self._check(self._lib.spt_progressive_temporal_begin(self._h, C.byref(p)))

    def progressive_temporal_demodulate(self, params=True):
        """Runs the temporal loop over illumination (spt_progressive_temporal_demodulate): ``params`` a ``DemodParams``, True for the
        default floor with the context's environment as background (as the C++ host's wrapper), or None / False to switch the mode off again.  Either way the history is dropped: the next frame starts a new one and
        the snapshots fail until it is made.  With the mode on every snapshot is remodulated under the last frame's albedo, coverage and
        emission."""
        self._prog_size("progressive_temporal_demodulate")
        if params is None or params is False:
            self._check(self._lib.spt_progressive_temporal_demodulate(self._h, None))
            return
        if params is True:                                   # the defaults, with the context's environment as the background
            params = DemodParams(background=self.environment())
        p = _demod_params(params)
        self._check(self._lib.spt_progressive_temporal_demodulate(self._h, C.byref(p)))

    def progressive_temporal_frame(self, samps_per_cell, seed, reset=False, camera=None):
        """One frame of the temporal loop (spt_progressive_temporal_frame): the radiance launch of ``progressive_frame`` and the feature
        launch of the same camera, samples and seed, blended into the history reprojected from the previous frame's camera; ``reset``
        drops the history.  Blocking; returns the radiance launch's stats.  The other accumulators are not touched."""
        w, h, _ = self._prog_size("progressive_temporal_frame")
        cam = camera if camera is not None else smallpt_camera(w, h)
        st = SptStats()
        self._check(self._lib.spt_progressive_temporal_frame(self._h, C.byref(cam), samps_per_cell, seed, 1 if reset else 0, C.byref(st)))
        return _stats_dict(st)

    def progressive_temporal_snapshot(self, var=False, length=False):
        """The temporal loop's picture: the (h, w, 3) float32 MEAN image (display weight 1); with ``var`` and / or ``length`` a tuple
        (mean[, (h, w) variance][, (h, w) history length])."""
        w, h, _ = self._prog_size("progressive_temporal_snapshot")
        out = np.empty((h, w, 3), dtype=np.float32)
        v = np.empty((h, w), dtype=np.float32) if var else None
        n = np.empty((h, w), dtype=np.float32) if length else None
        self._check(self._lib.spt_progressive_temporal_snapshot(self._h, out.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p) if var else None,
                                                                n.ctypes.data_as(C.c_void_p) if length else None))
        if not var and not length:
            return out
        return (out,) + ((v,) if var else ()) + ((n,) if length else ())

    def progressive_temporal_display_snapshot(self, params=None, denoise=None):
        """The temporal loop's picture as 8-bit colour straight from the device (spt_progressive_temporal_display_snapshot): the mean, or
        with ``denoise`` (a ``DenoiseParams``, or True for the defaults) the mean filtered under the last frame's guides, through
        ``display`` with ``params`` (weight 1 suits a mean).  Returns uint8 (h, w, 3|4)."""
        w, h, _ = self._prog_size("progressive_temporal_display_snapshot")
        dp = _display_params(params)
        out = np.empty((h, w, dp.channels), dtype=np.uint8)
        p = dp.as_c()
        fp = None if denoise is None or denoise is False else _denoise_params(None if denoise is True else denoise)
        self._check(self._lib.spt_progressive_temporal_display_snapshot(self._h, C.byref(fp) if fp is not None else None, C.byref(p),
                                                                        out.ctypes.data_as(C.c_void_p)))
        return out

    def progressive_temporal_denoised_var_snapshot(self, var_params=None, params=None, var_mean=False):
        """The temporal loop's mean under the variance-guided filter (spt_progressive_temporal_denoised_var_snapshot): the variance
        estimate of the current history (``var_params`` a ``TemporalVarParams``), then ``denoise_pvar`` of the mean under it and the last
        frame's guides (``params`` a ``DenoiseVarParams``).  Returns the (h, w, 3) float32 picture (display weight 1); with ``var_mean``
        a tuple (picture, the (h, w) variance of the mean it was filtered under).  Nothing of the loop changes."""
        w, h, _ = self._prog_size("progressive_temporal_denoised_var_snapshot")
        out = np.empty((h, w, 3), dtype=np.float32)
        vm = np.empty((h, w), dtype=np.float32) if var_mean else None
        vp, p = _temporal_var_params(var_params), _denoise_var_params(params)
        self._check(self._lib.spt_progressive_temporal_denoised_var_snapshot(self._h, C.byref(vp), C.byref(p), out.ctypes.data_as(C.c_void_p),
                                                                             vm.ctypes.data_as(C.c_void_p) if var_mean else None))
        return (out, vm) if var_mean else out

    def progressive_temporal_display_var_snapshot(self, params=None, var_params=None, denoise=None):
        """The same picture as 8-bit colour straight from the device (spt_progressive_temporal_display_var_snapshot): ``display`` with
        ``params`` (a ``DisplayParams``; weight 1 suits a mean) of the filtered mean; ``denoise`` a ``DenoiseVarParams`` or None for the
        defaults.  Returns uint8 (h, w, 3|4)."""
        w, h, _ = self._prog_size("progressive_temporal_display_var_snapshot")
        dp = _display_params(params)
        out = np.empty((h, w, dp.channels), dtype=np.uint8)
        p, vp, fp = dp.as_c(), _temporal_var_params(var_params), _denoise_var_params(denoise)
        self._check(self._lib.spt_progressive_temporal_display_var_snapshot(self._h, C.byref(vp), C.byref(fp), C.byref(p), out.ctypes.data_as(C.c_void_p)))
        return out

    def progressive_end(self):
        self._check(self._lib.spt_progressive_end(self._h))
        self._prog = None

    def _prog_size(self, who):
        prog = getattr(self, "_prog", None)
        if prog is None:
            raise SptError(f"{who}: call progressive_begin first")
        return prog

    def set_watchdog(self, seconds):
        """Pool kernel: a launch whose waves run longer than this fails in sync() instead of hanging (0 = off)."""
        self._check(self._lib.spt_set_watchdog(self._h, float(seconds)))
        self._state["watchdog"] = float(seconds)
        self._state_version += 1

    def last_kernel(self):
        """'pool' (spt_pool.hip, material-sorted), 'mega' (spt_kernel.hip), 'mesh' (spt_mesh.hip, triangles), 'sbvh' (spt_mesh.hip over a
        sphere hierarchy), 'gpool' (spt_gpool.hip, uniform grid over a large sphere table driven by wave-private path pools: the default above 24
        spheres), 'grid' (spt_grid.hip, the same grid with lanes that own their path: tables that leave no LDS for the pools) or 'mesh_inst' (spt_mesh.hip
        over an instanced scene, spt_set_instances) for the last launch."""
        return {0: "mega", 1: "pool", 2: "mesh", 3: "sbvh", 4: "grid", 5: "gpool", 6: "mesh_bvh", 7: "mesh_bvh_fast", 8: "mesh_inst"}[self._lib.spt_last_kernel(self._h)]

    def grid_placement(self):
        """Where the grid kernels of the current sphere scene read their tables (spt_grid_placement): 0 = everything staged in LDS,
        1 = everything from global memory, 2 = the sphere records from global memory and the grid tables in LDS; -1 = no grid."""
        return int(self._lib.spt_grid_placement(self._h))

    def set_line_form(self, form=0):
        """How the structures of mesh scenes built from now on keep their thin triangles (csrc/spt_internal.h spt_set_line_form): 0 = by
        their number (the default), 1 = the table, 2 = the cone tree.  Results never depend on it."""
        self._check(self._lib.spt_set_line_form(self._h, int(form)))
        self._state["line_form"] = int(form)
        self._state_version += 1

    def mesh_line_form(self):
        """(form, thin triangles) of the current mesh scene's built structures (spt_mesh_line_form): form 0 = none, 1 = table, 2 = tree."""
        n = C.c_uint32(0)
        return int(self._lib.spt_mesh_line_form(self._h, C.byref(n))), int(n.value)

    def render_interleaved_device(self, out_tensor, w, h, block_rows, world, rank, samps_per_cell, seed=0,
                                  normalise=False, camera=None, stream=None):
        """Like render_rows_device for the rows of rank `rank` when the image is dealt out to `world` ranks round-robin in
        blocks of `block_rows` rows (spt_render_interleaved_device); out_tensor holds those rows packed in ascending order."""
        rows = int(self._lib.spt_interleaved_row_count(h, block_rows, world, rank))
        if out_tensor.numel() != rows * w * 3 or not out_tensor.is_contiguous():
            raise ValueError(f"out_tensor must be contiguous with {rows}*w*3 float32 elements")
        if str(out_tensor.dtype) != "torch.float32" or out_tensor.device.type != "cuda":
            raise ValueError("out_tensor must be a float32 tensor on the GPU")
        cam = camera if camera is not None else smallpt_camera(w, h)
        self._check(self._lib.spt_render_interleaved_device(
            self._h, C.byref(cam), w, h, block_rows, world, rank, samps_per_cell, seed,
            FLAG_NORMALISE if normalise else 0, C.c_void_p(out_tensor.data_ptr()), C.c_void_p(stream) if stream else None))

    def diag(self):
        """Phase timings / lane counters of the last launch of the instrumented build (variant bit 8)."""
        arr = (C.c_uint64 * 24)()
        self._check(self._lib.spt_diag(self._h, C.byref(arr)))
        return [int(v) for v in arr]

    def chunk_order(self):
        """The pool kernel's chunk order for the next launch of the same view (spt_chunk_order_snapshot): a permutation of the
        64-task chunks, most expensive first; empty when the last launch recorded none."""
        cap = 1 << 22
        buf = np.empty(cap, dtype=np.uint32)
        n = C.c_uint32(0)
        self._check(self._lib.spt_chunk_order_snapshot(self._h, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return buf[:n.value].copy()

    def selftest_math(self, op, x, w=1024):
        """Runs device helper `op` over the float32 array x (see spt_selftest_math)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        self._check(self._lib.spt_selftest_math(self._h, int(op), x.ctypes.data_as(C.c_void_p),
                                                out.ctypes.data_as(C.c_void_p), x.size, int(w)))
        return out

    def sync(self):
        st = SptStats()
        self._check(self._lib.spt_sync(self._h, C.byref(st)))
        return _stats_dict(st)


class MultiRenderer:
    """spt_multi_* (include/smallpt_mi355x_multi.h): ONE process, one host thread + context per device, row bands,
    RCCL exchange into the root device's framebuffer.  `self_exchange` routes a single device's band through RCCL too
    (rehearsal of the exchange step on a one-GPU box)."""

    SELF_EXCHANGE, CONTIGUOUS, COPY_EXCHANGE = 1, 2, 4

    def __init__(self, device_ids=(0,), self_exchange=False, contiguous=False, copy_exchange=False):
        self._lib = load_multi_library()
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        h = C.c_void_p()
        flags = (self.SELF_EXCHANGE if self_exchange else 0) | (self.CONTIGUOUS if contiguous else 0) | (self.COPY_EXCHANGE if copy_exchange else 0)
        if self._lib.spt_multi_create(ids, len(device_ids), flags, C.byref(h)):
            raise SptError(self._lib.spt_multi_last_error(None).decode())
        self._h = h
        self.device_ids = tuple(int(d) for d in device_ids)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.spt_multi_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise SptError(self._lib.spt_multi_last_error(self._h).decode())

    def set_scene(self, spheres):
        spheres = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
        self._check(self._lib.spt_multi_set_scene(self._h, spheres.ctypes.data_as(C.c_void_p), len(spheres)))

    def set_meshes(self, meshes, materials):
        """spt_multi_set_meshes: the triangle scene on every device (see Renderer.set_meshes)."""
        ms = (SptMesh * max(1, len(meshes)))()
        mats = (SptMaterial * max(1, len(meshes)))()
        self._mesh_keepalive = list(meshes)
        for i, (m, (e, col, refl)) in enumerate(zip(meshes, materials)):
            ms[i].positions, ms[i].normals, ms[i].indices = m.positions.ctypes.data, m.normals.ctypes.data, m.indices.ctypes.data
            ms[i].nverts, ms[i].ntris = len(m.positions), len(m.indices)
            mats[i].emission = (C.c_float * 3)(*[float(v) for v in e])
            mats[i].color = (C.c_float * 3)(*[float(v) for v in col])
            mats[i].refl = int(refl)
        self._check(self._lib.spt_multi_set_meshes(self._h, ms, len(meshes), mats))

    def set_mesh_accel(self, accel):
        self._check(self._lib.spt_multi_set_mesh_accel(self._h, int(accel)))

    def set_sphere_accel(self, accel):
        self._check(self._lib.spt_multi_set_sphere_accel(self._h, int(accel)))

    def set_environment(self, rgb):
        """spt_multi_set_environment: Renderer.set_environment on every device."""
        e = environment_radiance(rgb)
        self._check(self._lib.spt_multi_set_environment(self._h, e.ctypes.data_as(C.POINTER(C.c_float))))

    def set_rank_watchdog(self, rank, seconds):
        """Test hook (csrc/spt_internal.h): kernel watchdog of one rank's context."""
        self._check(self._lib.spt_multi_set_rank_watchdog(self._h, int(rank), float(seconds)))

    def inject_exchange_failure(self, rank):
        """Test hook (csrc/spt_internal.h): `rank` fails inside its part of the next RCCL exchange."""
        self._check(self._lib.spt_multi_inject_exchange_failure(self._h, int(rank)))

    def render(self, w, h, samps_per_cell, seed=0, normalise=False, camera=None, to_host=True):
        """Returns ((h, w, 3) float32 image or None, stats dict); with to_host=False the framebuffer stays on the root
        device (``framebuffer_ptr()``)."""
        cam = camera if camera is not None else smallpt_camera(w, h)
        out = np.empty((h, w, 3), dtype=np.float32) if to_host else None
        st = SptMultiStats()
        self._check(self._lib.spt_multi_render(self._h, C.byref(cam), w, h, samps_per_cell, seed,
                                               FLAG_NORMALISE if normalise else 0,
                                               out.ctypes.data_as(C.c_void_p) if to_host else None, C.byref(st)))
        return out, {"samples": int(st.samples), "bounces": int(st.bounces), "max_depth_kills": int(st.max_depth_kills),
                     "render_ms": float(st.render_ms), "gather_ms": float(st.gather_ms), "total_ms": float(st.total_ms),
                     "ndev": int(st.ndev)}

    def framebuffer_ptr(self):
        return self._lib.spt_multi_framebuffer(self._h)

    # the viewer's render loop over all devices (spt_multi_progressive_*): accumBuffer on the root device
    def progressive_begin(self, w, h):
        self._check(self._lib.spt_multi_progressive_begin(self._h, w, h))
        self._prog = (w, h)

    def progressive_frame(self, samps_per_cell, seed, clear=False, camera=None):
        """outImage = render(camera, ..., seed) on all devices; accumBuffer = outImage (clear) or += outImage on the root."""
        w, h = self._prog
        cam = camera if camera is not None else pinhole_camera()
        st = SptMultiStats()
        self._check(self._lib.spt_multi_progressive_frame(self._h, C.byref(cam), samps_per_cell, seed, 1 if clear else 0, C.byref(st)))
        return {"samples": int(st.samples), "bounces": int(st.bounces), "render_ms": float(st.render_ms), "gather_ms": float(st.gather_ms), "ndev": int(st.ndev)}

    def progressive_snapshot(self):
        w, h = self._prog
        out = np.empty((h, w, 3), dtype=np.float32)
        self._check(self._lib.spt_multi_progressive_snapshot(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def progressive_end(self):
        self._check(self._lib.spt_multi_progressive_end(self._h))


class ProgressiveRenderer:
    """The viewer's render-thread loop (smallpt.cpp:895-942) with the accumulation buffer resident in HBM:
    every ``step()`` renders one frame with seed = frame counter (:893,922,926) as an un-normalised sum
    (Renderer::render convention), adds it to the accumulation tensor (:935) and returns the display weight
    1/(frames*spp) of :957.  ``update_camera`` mirrors the "update_camera" request (:911-916): new camera,
    the next frame is still rendered with the RUNNING frame counter as its seed (:922), replaces the buffer
    (:931-935), and only then is the counter reset to 1 (:938-939).

    ``pipeline=2`` keeps two frames in flight on two contexts/streams of the same device: frame k+1 starts while the
    last, longest paths of frame k are still finishing (the end of a 4-spp frame is a handful of mirror<->glass chains,
    DESIGN.md section 5), the accumulation kernels stay in frame order (stream events), so ``accum`` is bit-identical
    to the serial loop; ``step()`` then returns without waiting and ``flush()`` waits for everything in flight."""

    def __init__(self, renderer, w, h, samps_per_cell, camera=None, pipeline=1):
        import torch
        self.r, self.w, self.h, self.samps = renderer, w, h, samps_per_cell
        self.camera = camera if camera is not None else pinhole_camera()
        dev = torch.device("cuda", renderer.device_id)
        self.accum = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        self.frames = 0          # sampleCount, smallpt.cpp:893
        self._clear = True       # the zero-initialised accumBuffer (:882): replacing it == adding to zeros
        self.pipeline = max(1, int(pipeline))
        self._lanes = []
        for i in range(self.pipeline):
            rr = renderer if i == 0 else Renderer(renderer.device_id)
            if i:
                renderer.replay_state_on(rr)              # spheres OR meshes + materials, closest-hit modes, tuning, watchdog
            self._lanes.append({"r": rr, "version": renderer._state_version, "frame": torch.empty((h, w, 3), dtype=torch.float32, device=dev),
                                # alternate stream priorities: HIP maps equal-priority streams of a process onto a shared hardware queue,
                                # which would serialise the two frames
                                "stream": torch.cuda.current_stream(dev) if self.pipeline == 1 else torch.cuda.Stream(dev, priority=-(i % 2)),
                                "done": None})
        self.frame = self._lanes[0]["frame"]
        self._issued = 0
        self._last_acc = None    # event after the most recent accumulation kernel
        self._last_seed = None
        self._aov_names = None   # aov_begin: the selected feature buffers (accumulated behind the C-ABI, spt_progressive_aov_*)

    def update_camera(self, camera):
        self.camera = camera
        self._clear = True

    def step(self):
        import torch
        lane = self._lanes[self._issued % self.pipeline]
        self._issued += 1
        r, stream = lane["r"], lane["stream"]
        if r is not self.r and lane["version"] != self.r._state_version:      # the primary's scene / modes changed since this lane was set up
            lane["stream"].synchronize()
            r.sync()
            self.r.replay_state_on(r)
            lane["version"] = self.r._state_version
        seed = self.frames       # :922 renders with the running sampleCount, also on the clearing frame
        self._last_seed = seed
        if self.pipeline > 1 and lane["done"] is not None:
            stream.wait_event(lane["done"])               # the lane's frame buffer was read by its last accumulation
        r.render_rows_device(lane["frame"], self.w, self.h, 0, self.h, self.samps, seed=seed, normalise=False,
                             camera=self.camera, stream=stream.cuda_stream)
        if self.pipeline > 1 and self._last_acc is not None:
            stream.wait_event(self._last_acc)             # accumulations stay in frame order
        r._check(r._lib.spt_accumulate_device(r._h, C.c_void_p(self.accum.data_ptr()), C.c_void_p(lane["frame"].data_ptr()),
                                               self.accum.numel(), 1 if self._clear else 0, C.c_void_p(stream.cuda_stream)))
        if self.pipeline > 1:
            ev = torch.cuda.Event()
            ev.record(stream)
            lane["done"] = self._last_acc = ev
        self.frames = 1 if self._clear else self.frames + 1
        self._clear = False
        if self.pipeline == 1:
            r.sync()
        return 1.0 / (self.frames * 4 * self.samps)

    def flush(self):
        """Waits for every frame in flight (needed before reading ``accum`` when pipeline > 1)."""
        for lane in self._lanes:
            lane["stream"].synchronize()
            lane["r"].sync()

    def aov_begin(self, kinds=("normal",)):
        """Feature buffers beside the radiance loop -- the reference's viewer as shipped accumulates the first hit's normal --: one
        device-resident accumulation buffer per kind of ``kinds`` (names as ``Renderer.render_aov_set``), zeroed."""
        mask, names = _aov_set(kinds)
        r = self.r
        if self._aov_names is None:
            # spt_progressive_aov_begin takes the image size from spt_progressive_begin, whose own radiance accumBuffer and frame (2 x w*h*3
            # floats on the device) stay unused here: this class accumulates radiance in its torch tensor.  Freed by close().
            r._check(r._lib.spt_progressive_begin(r._h, self.w, self.h))
        r._check(r._lib.spt_progressive_aov_begin(r._h, mask))
        self._aov_names = names

    def aov_frame(self, seed=None, clear=False):
        """One fused launch of the selected buffers (un-normalised sums) for the current camera, added to (``clear``: replacing) their
        accumulation buffers; blocking.  seed None = the seed of the radiance frame ``step()`` issued last, so that beauty and features
        are those of the same samples.  Returns the stats."""
        if self._aov_names is None:
            raise SptError("aov_frame: call aov_begin first")
        if seed is None:
            seed = 0 if self._last_seed is None else self._last_seed
        self.flush()
        st = SptStats()
        r = self.r
        r._check(r._lib.spt_progressive_aov_frame(r._h, C.byref(self.camera), self.samps, seed, 1 if clear else 0, C.byref(st)))
        return _stats_dict(st)

    def aov_snapshot(self, kind):
        """The accumulation buffer of one selected kind: (h, w, 3) float32."""
        if self._aov_names is None or kind not in self._aov_names:
            raise ValueError(f"aov_snapshot: {kind!r} is not one of the kinds given to aov_begin")
        out = np.empty((self.h, self.w, 3), dtype=np.float32)
        r = self.r
        r._check(r._lib.spt_progressive_aov_snapshot(r._h, 1 << AOV_SET_KINDS[kind], out.ctypes.data_as(C.c_void_p)))
        return out

    def close(self):
        self.flush()
        if self._aov_names is not None:
            self.r._check(self.r._lib.spt_progressive_end(self.r._h))
            self._aov_names = None
        for lane in self._lanes[1:]:
            lane["r"].close()


def to_int(x):
    """toInt, smallpt.cpp:52."""
    return load_library().spt_to_int(float(x))


def write_ppm(path, rgb):
    """flipY + writeImage (smallpt.cpp:125-142) for an (h, w, 3) float32 image, row 0 = bottom."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w, _ = rgb.shape
    if load_library().spt_write_ppm(str(path).encode(), rgb.ctypes.data_as(C.c_void_p), w, h):
        raise SptError(f"cannot write {path}")


def display_thresholds():
    """The 255 float32 thresholds T[1..255] of toInt (spt_display_thresholds): T[k] = the smallest float with toInt >= k."""
    out = np.empty(255, dtype=np.float32)
    if load_library().spt_display_thresholds(out.ctypes.data_as(C.c_void_p)):
        raise SptError("spt_display_thresholds: toInt is not monotone on this machine")
    return out


def display_quantise_host(v):
    """The display transform's table count on the CPU (spt_display_quantise_host): uint8 of v's shape, == toInt(v), NaN -> 0."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    out = np.empty(v.shape, dtype=np.uint8)
    if load_library().spt_display_quantise_host(v.ctypes.data_as(C.c_void_p), v.size, out.ctypes.data_as(C.c_void_p)):
        raise SptError("spt_display_quantise_host failed")
    return out


def write_ppm_rgb8(path, rgb8):
    """writeImage (smallpt.cpp:136-142) for an (h, w, 3) uint8 image whose row 0 is the TOP row (``display`` with ``flip_y``)."""
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    if rgb8.ndim != 3 or rgb8.shape[2] != 3:
        raise ValueError("write_ppm_rgb8: one (h, w, 3) uint8 image")
    h, w, _ = rgb8.shape
    if load_library().spt_write_ppm_rgb8(str(path).encode(), rgb8.ctypes.data_as(C.c_void_p), w, h):
        raise SptError(f"cannot write {path}")
