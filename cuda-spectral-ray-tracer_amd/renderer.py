"""Device renderer handle (srt_ctx): the `renderer` / render_manager::step pair of the reference
(rendering/rendering.cuh:39-155, rendering/render_manager.cu:3-66) over the C-ABI.  All compute happens in
libsrt_hip.so on the GPU; this module only moves pointers."""
import contextlib
import ctypes as C

import numpy as np

from . import binding as B
from .scene import ray_segments, refit_vertices

DEFAULT_TX, DEFAULT_TY = 28, 16   # render_manager.cu:93-94
FEATURE_CHANNELS = 8              # first-hit sums per pixel: normal xyz, albedo rgb, distance, hits (srt_c_api.h, srt_accum_reset_features)
FILM_SAMPLES = 95                 # the spectral film's grid: 360 + 5 j nm, j = 0 .. 94 (srt_c_api.h, srt_accum_reset_spectral)


def reference_grid(chunk_w, chunk_h, tx=DEFAULT_TX, ty=DEFAULT_TY):
    """blocks = (w/28+1, h/16+1), render_manager.cu:96"""
    return chunk_w // tx + 1, chunk_h // ty + 1


FLT_MAX = float(np.finfo(np.float32).max)


def ray_batch(origins, directions, tmin=0.0, tmax=None):
    """The (n, 8) float32 rows of the ray queries (Renderer.intersect / occluded): ox oy oz tmin dx dy dz tmax.  origins and directions
    (n, 3) -- or one origin (3,) for all --, tmin and tmax scalars or n values; tmax None means FLT_MAX.  numpy inputs give a numpy array, a
    torch tensor among origins / directions gives a tensor on its device."""
    if tmax is None:
        tmax = FLT_MAX
    tensor = next((a for a in (origins, directions) if not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")), None)
    if tensor is not None:
        import torch
        dev = tensor.device
        d = torch.as_tensor(directions, dtype=torch.float32, device=dev)
        if d.dim() != 2 or d.shape[1] != 3:
            raise ValueError("ray_batch: directions must have shape (n, 3), got %r" % (tuple(d.shape),))
        rows = torch.empty((d.shape[0], 8), dtype=torch.float32, device=dev)
        rows[:, 0:3] = torch.as_tensor(origins, dtype=torch.float32, device=dev)
        rows[:, 3] = torch.as_tensor(tmin, dtype=torch.float32, device=dev)
        rows[:, 4:7] = d
        rows[:, 7] = torch.as_tensor(tmax, dtype=torch.float32, device=dev)
        return rows
    d = np.asarray(directions, np.float32)
    if d.ndim != 2 or d.shape[1] != 3:
        raise ValueError("ray_batch: directions must have shape (n, 3), got %r" % (d.shape,))
    rows = np.empty((d.shape[0], 8), np.float32)
    rows[:, 0:3] = np.asarray(origins, np.float32)
    rows[:, 3] = np.asarray(tmin, np.float32)
    rows[:, 4:7] = d
    rows[:, 7] = np.asarray(tmax, np.float32)
    return rows


class Renderer:
    def __init__(self, device=0, _borrowed=None):
        if _borrowed is not None:            # a context owned by a communicator (srt_comm_init_all)
            self._h, self._owned = C.c_void_p(_borrowed), False
            self.device = B.lib().srt_ctx_device(self._h)
        else:
            h = C.c_void_p()
            B.check(B.lib().srt_create(int(device), C.byref(h)))
            self._h, self._owned = h, True
            self.device = device
        self.geom = None
        self.gather_planes = 3

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                B.lib().srt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, code):
        return B.check(code, self._h)

    def upload_scene(self, scene):
        self._ck(B.lib().srt_upload_scene(self._h, scene.handle))

    def launch_plan(self):
        """dict(waves_per_cu, n_cached, all_cached, narrow_refs, paired) of the uploaded scene's render launch"""
        w, n, a, r = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._ck(B.lib().srt_launch_plan(self._h, C.byref(w), C.byref(n), C.byref(a), C.byref(r)))
        pr = C.c_int()
        self._ck(B.lib().srt_launch_paired(self._h, C.byref(pr)))
        return dict(waves_per_cu=w.value, n_cached=n.value, all_cached=bool(a.value), narrow_refs=bool(r.value), paired=bool(pr.value), test_knobs=self.test_knobs())

    def set_test_knobs(self, wide_refs=False, lds_cache_max=-1, lane_limit=0):
        """tests / tools only (srt_c_api.h): force kernel variants the plan would not pick; upload the scene again afterwards"""
        self._ck(B.lib().srt_set_test_knobs(self._h, 1 if wide_refs else 0, int(lds_cache_max), int(lane_limit)))

    def test_knobs(self):
        w, m, l, e = C.c_int(), C.c_int(), C.c_uint32(), C.c_int()
        self._ck(B.lib().srt_get_test_knobs(self._h, C.byref(w), C.byref(m), C.byref(l), C.byref(e)))
        return dict(wide_refs=bool(w.value), lds_cache_max=m.value, lane_limit=l.value, from_env=bool(e.value))

    def set_camera(self, cam):
        self._ck(B.lib().srt_set_camera(self._h, C.byref(cam)))

    def refit(self, vertices):
        """BVH refit on the device (srt_refit_vertices / srt_refit_vertices_dev): new vertices (n_tris, 3, 3) float32 for the uploaded
        scene, its topology kept -- no scene build, no upload.  A numpy array goes through the host entry; a torch tensor must live on
        this renderer's device, be contiguous and float32, and goes through the device-pointer entry without visiting the host (its
        stream is waited for first).  Shapes and dtypes are checked here, before any device is touched.  Afterwards the accumulation
        and the temporal history are invalid, as after upload_scene (a renderer that tracks motion keeps the history: track_motion);
        camera and device parameters stay."""
        if isinstance(vertices, np.ndarray):
            v = refit_vertices("Renderer.refit", vertices)
            self._ck(B.lib().srt_refit_vertices(self._h, B.fptr(v), v.shape[0]))
            return
        t = vertices
        if not all(hasattr(t, a) for a in ("data_ptr", "is_contiguous", "device", "dtype", "shape")):
            raise TypeError("Renderer.refit: vertices must be a numpy array or a torch tensor (n_tris, 3, 3) float32, got %r" % type(t).__name__)
        import torch
        if t.dtype != torch.float32:
            raise TypeError("Renderer.refit: the tensor must be float32, got %s" % t.dtype)
        if t.dim() != 3 or tuple(t.shape[1:]) != (3, 3) or t.shape[0] == 0:
            raise ValueError("Renderer.refit: the tensor must have shape (n_tris, 3, 3) with n_tris >= 1, got %r" % (tuple(t.shape),))
        if t.device.type != "cuda" or (t.device.index or 0) != self.device:
            raise ValueError("Renderer.refit: the tensor lives on %s, the renderer on GPU %d" % (t.device, self.device))
        if not t.is_contiguous():
            raise ValueError("Renderer.refit: the tensor must be contiguous")
        torch.cuda.current_stream(t.device).synchronize()      # (the entry works on the NULL stream: the tensor must be complete)
        self._ck(B.lib().srt_refit_vertices_dev(self._h, C.c_void_p(t.data_ptr()), t.shape[0]))

    def refit_last_ms(self):
        """kernel-only ms of the context's last refit (srt_refit_last_ms): dict(triangles, levels, n_levels)"""
        a, b, n = C.c_float(), C.c_float(), C.c_uint32()
        self._ck(B.lib().srt_refit_last_ms(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return dict(triangles=a.value, levels=b.value, n_levels=n.value)

    def scene_image(self, which):
        """read-back of one scene image (srt_read_scene_image; tests and tools): which = "nodes", "nodes_sw", "fringe", "tris" or "shade"
        -> its words as a uint32 array, empty for an image the launch plan does not keep.  Synchronises, only reads."""
        if which not in B.SCENE_IMAGES:
            raise ValueError("scene_image: unknown image %r (%s)" % (which, ", ".join(B.SCENE_IMAGES)))
        n = C.c_size_t()
        self._ck(B.lib().srt_read_scene_image(self._h, B.SCENE_IMAGES[which], None, 0, C.byref(n)))
        out = np.zeros(n.value // 4, np.uint32)
        if out.size:
            self._ck(B.lib().srt_read_scene_image(self._h, B.SCENE_IMAGES[which], out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(n)))
        return out

    def init_device_params(self, chunk_w, chunk_h, spp, bounce_limit, seed=1984, tx=DEFAULT_TX, ty=DEFAULT_TY, bx=None, by=None):
        if bx is None or by is None:
            bx, by = reference_grid(chunk_w, chunk_h, tx, ty)
        self._ck(B.lib().srt_init_device_params(self._h, tx, ty, bx, by, chunk_w, chunk_h, spp, bounce_limit, seed))
        self.geom = dict(tx=tx, ty=ty, bx=bx, by=by, chunk_w=chunk_w, chunk_h=chunk_h, n_lanes=tx * ty * bx * by)

    def set_partition(self, rank, world):
        self._ck(B.lib().srt_set_partition(self._h, rank, world))

    def set_count_traversal(self, on):
        self._ck(B.lib().srt_set_count_traversal(self._h, 1 if on else 0))

    def render_chunk(self, width, height, offx=0, offy=0, stream=None):
        self._ck(B.lib().srt_render_chunk(self._h, width, height, offx, offy, C.c_void_p(stream or 0)))

    def synchronize(self):
        self._ck(B.lib().srt_synchronize(self._h))

    def accum_reset(self):
        """start a progressive accumulation: zero the per-pixel XYZ sums and the sample total (the RNG streams are not re-seeded)"""
        self._ck(B.lib().srt_accum_reset(self._h))

    def render_chunk_accum(self, width, height, spp_add, offx=0, offy=0, stream=None):
        """add spp_add samples per pixel to the accumulation and write the running mean to the tile buffer (srt_c_api.h): after
        accum_reset, passes of s1 .. sk samples equal one render_chunk of s1 + .. + sk samples bit for bit"""
        self._ck(B.lib().srt_render_chunk_accum(self._h, width, height, offx, offy, spp_add, C.c_void_p(stream or 0)))

    @property
    def accum_samples(self):
        """samples per pixel the accumulation holds (0 after accum_reset, or when there is none)"""
        n = C.c_uint32()
        self._ck(B.lib().srt_accum_samples(self._h, C.byref(n)))
        return n.value

    def accum_reset_adaptive(self, rel_tol, abs_tol=0.0, min_spp=16):
        """start an ADAPTIVE accumulation (srt_c_api.h): like accum_reset, and each later pass adds its samples only to the pixels that
        have not converged -- a pixel stops once the variance of its mean luminance is at most (rel_tol * mean + abs_tol)^2, after at
        least min_spp samples.  A pixel that stopped after n samples holds exactly the plain n-spp render's value."""
        self._ck(B.lib().srt_accum_reset_adaptive(self._h, C.byref(adaptive_config(rel_tol, abs_tol, min_spp))))

    @property
    def accum_active(self):
        """pixels of this rank still active after the last adaptive pass (0 before the first pass); synchronises"""
        n = C.c_uint64()
        self._ck(B.lib().srt_accum_active(self._h, C.byref(n)))
        return n.value

    def accum_stats(self, image_width, image_height):
        """row-major maps of the adaptive accumulation's chunk: dict(samples=uint32, sum_y=float32, sum_y2=float32), each of
        image_width * image_height entries; only the chunk's rectangle is written (zeros elsewhere, and at pixels of other ranks)"""
        n = image_width * image_height
        samples, sum_y, sum_y2 = np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        self._ck(B.lib().srt_read_accum_stats(self._h, samples.ctypes.data_as(C.POINTER(C.c_uint32)), B.fptr(sum_y), B.fptr(sum_y2),
                                              image_width, image_height))
        return dict(samples=samples, sum_y=sum_y, sum_y2=sum_y2)

    def accum_reset_spectral(self):
        """start a SPECTRAL accumulation (srt_c_api.h): like accum_reset, and each later pass also adds every path's seven powers to
        the pixel's film, 95 raw float32 sums on the 5 nm CIE grid (read_spectral; spectral_radiance normalises them).  Never adaptive:
        accum_reset_adaptive_spectral is the adaptive one."""
        self._ck(B.lib().srt_accum_reset_spectral(self._h))

    def read_spectral(self, image_width, image_height, first=0, count=FILM_SAMPLES, into=None):
        """raw film sums of grid samples [first, first + count) as float32 (image_height, image_width, count): only the chunk's
        rectangle is written (zeros elsewhere, and at pixels of other ranks)"""
        out = np.zeros((image_height, image_width, count), np.float32) if into is None else into
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == image_width * image_height * count
        self._ck(B.lib().srt_read_spectral(self._h, int(first), int(count), B.fptr(out), image_width, image_height))
        return out

    def develop_spectral(self, image_width, image_height, response, scale=1.0, filter=None):
        """the film developed on the device (srt_develop_spectral): out[y, x, k] = (sum over j ascending of F_j * response[k][j]) * scale
        in float32, (image_height, image_width, K) -- another sensor's curves, a colour filter (folded into the curves by
        sensor_response), a band image.  Only the K planes leave the device; placement as read_spectral (the chunk's rectangle, zeros
        elsewhere and at pixels of other ranks).  Reads the accumulation, changes nothing of it."""
        resp = sensor_response(response, filter)
        s = _develop_scale(scale)
        out = np.zeros((image_height, image_width, resp.shape[0]), np.float32)
        self._ck(B.lib().srt_develop_spectral(self._h, B.fptr(resp), resp.shape[0], s, B.fptr(out), image_width, image_height))
        return out

    def develop_spectral_srgb(self, image_width, image_height, response=None, scale=None, filter=None):
        """three developed channels taken as XYZ sums (srt_develop_spectral_srgb): dict(xyz, lin, fb) of (image_height, image_width, 3)
        float32 arrays -- the developed sums, and the unquantised and quantised sRGB the render kernel's conversion makes of them and the
        accumulation's sample total.  response=None: the colour-matching rows of srt_color_tables; scale=None: the kernel's float32
        470/7, with which the sums are the film's own XYZ sums up to reassociation.  filter: 95 transmittances in front of the lens."""
        if response is None and filter is None:
            resp, ptr = None, None
        else:
            resp = sensor_response(cie_response() if response is None else response, filter)
            if resp.shape[0] != 3:
                raise ValueError("develop_spectral_srgb: needs three response curves (taken as X, Y, Z), got %d" % resp.shape[0])
            ptr = B.fptr(resp)
        s = CIE_SCALE if scale is None else _develop_scale(scale)
        out = [np.zeros((image_height, image_width, 3), np.float32) for _ in range(3)]
        self._ck(B.lib().srt_develop_spectral_srgb(self._h, ptr, s, B.fptr(out[0]), B.fptr(out[1]), B.fptr(out[2]), image_width, image_height))
        return dict(xyz=out[0], lin=out[1], fb=out[2])

    def develop_kat(self, film, response, scale=1.0):
        """the develop kernel on an explicit film (srt_develop_kat): film (n_pixels, 95) float32 -> (n_pixels, K).  Needs no scene and no
        accumulation."""
        resp = sensor_response(response)
        s = _develop_scale(scale)
        rows = np.ascontiguousarray(film, np.float32)
        if rows.ndim != 2 or rows.shape[1] != FILM_SAMPLES or rows.shape[0] == 0:
            raise ValueError("develop_kat: needs a film (n_pixels, %d) with n_pixels >= 1, got %r" % (FILM_SAMPLES, rows.shape))
        out = np.zeros((rows.shape[0], resp.shape[0]), np.float32)
        self._ck(B.lib().srt_develop_kat(self._h, B.fptr(rows), rows.shape[0], B.fptr(resp), resp.shape[0], s, B.fptr(out)))
        return out

    def develop_last_ms(self):
        """kernel-only ms of the last develop on this context (srt_develop_last_ms): dict(contract, epilogue); epilogue is 0 unless it was
        develop_spectral_srgb"""
        a, b = C.c_float(), C.c_float()
        self._ck(B.lib().srt_develop_last_ms(self._h, C.byref(a), C.byref(b)))
        return dict(contract=a.value, epilogue=b.value)

    def meter(self, with_hist=False, **cfg):
        """the luminance histogram of the context's accumulation, of any kind, taken on the device, and the exposure decided from it
        (srt_meter_accum; cfg: the keywords of meter_config): dict(metered, dark, nonfinite, bin_ref, y_ref, gain) -- with
        with_hist=True also hist, the 4096 uint32 counts.  Under a partition only this rank's tiles are counted.  Reads the
        accumulation, changes nothing of it."""
        m, res = meter_config(**cfg), B.MeterResult()
        hist = np.zeros(METER_BINS, np.uint32) if with_hist else None
        self._ck(B.lib().srt_meter_accum(self._h, C.byref(m), None if hist is None else hist.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(res)))
        return _meter_dict(res, hist)

    def meter_kat(self, xyz_mean, with_hist=False, **cfg):
        """the meter kernel on an explicit XYZ-mean image (srt_meter_kat): xyz_mean (h, w, 3) float32 -- a denoised or developed picture,
        or a synthetic one -- -> the dict of meter().  Needs no scene and no accumulation."""
        m, res = meter_config(**cfg), B.MeterResult()
        img = _xyz_image("meter_kat", xyz_mean)
        hist = np.zeros(METER_BINS, np.uint32) if with_hist else None
        self._ck(B.lib().srt_meter_kat(self._h, C.byref(m), B.fptr(img), img.shape[1], img.shape[0],
                                       None if hist is None else hist.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(res)))
        return _meter_dict(res, hist)

    def expose(self, image_width, image_height, gain=None, **cfg):
        """the accumulation's picture at a metered (gain=None) or given exposure, through a tone curve and the usual conversion to sRGB, on
        the device (srt_expose_accum; cfg: the keywords of meter_config and of tone_config, told apart by name): dict(xyz, lin, fb) of
        (image_height, image_width, 3) float32 arrays -- the toned XYZ, its unquantised and its quantised sRGB, written in the chunk's
        rectangle only -- plus meter (the dict of meter(), None when a gain was given) and clip = dict(blown, crushed, nonfinite).
        Reads the accumulation, changes nothing of it."""
        mcfg, tcfg = _split_expose_cfg(cfg)
        meter = None
        if gain is None:
            tone_config(gain=1.0, **tcfg)          # (a bad tone is an error before the device is touched)
            meter = self.meter(**mcfg)
            gain = meter["gain"]
        elif mcfg:
            raise ValueError("expose: %s given with an explicit gain, which is not metered" % ", ".join(sorted(mcfg)))
        t, res = tone_config(gain=gain, **tcfg), B.ToneResult()
        out = [np.zeros((image_height, image_width, 3), np.float32) for _ in range(3)]
        self._ck(B.lib().srt_expose_accum(self._h, C.byref(t), B.fptr(out[0]), B.fptr(out[1]), B.fptr(out[2]), C.byref(res), image_width, image_height))
        return dict(xyz=out[0], lin=out[1], fb=out[2], meter=meter, clip=dict(blown=res.blown, crushed=res.crushed, nonfinite=res.nonfinite))

    def expose_kat(self, xyz_mean, gain=None, **cfg):
        """expose() on an explicit XYZ-mean image (srt_meter_kat when gain is None, then srt_expose_kat): xyz_mean (h, w, 3) float32 -> the
        dict of expose() with (h, w, 3) images.  Needs no scene and no accumulation."""
        mcfg, tcfg = _split_expose_cfg(cfg)
        img = _xyz_image("expose_kat", xyz_mean)
        meter = None
        if gain is None:
            tone_config(gain=1.0, **tcfg)
            meter = self.meter_kat(img, **mcfg)
            gain = meter["gain"]
        elif mcfg:
            raise ValueError("expose_kat: %s given with an explicit gain, which is not metered" % ", ".join(sorted(mcfg)))
        t, res = tone_config(gain=gain, **tcfg), B.ToneResult()
        out = [np.zeros(img.shape, np.float32) for _ in range(3)]
        self._ck(B.lib().srt_expose_kat(self._h, C.byref(t), B.fptr(img), img.shape[1], img.shape[0], B.fptr(out[0]), B.fptr(out[1]), B.fptr(out[2]), C.byref(res)))
        return dict(xyz=out[0], lin=out[1], fb=out[2], meter=meter, clip=dict(blown=res.blown, crushed=res.crushed, nonfinite=res.nonfinite))

    def expose_last_ms(self):
        """kernel-only ms of the context's last meter kernel and last tone kernel (srt_expose_last_ms): dict(meter, tone), 0 for one that
        has not run"""
        a, b = C.c_float(), C.c_float()
        self._ck(B.lib().srt_expose_last_ms(self._h, C.byref(a), C.byref(b)))
        return dict(meter=a.value, tone=b.value)

    def present(self, image_width, image_height, source="accum", gain=None, **cfg):
        """the accumulation's picture presented on the device (srt_present; the arguments of present_config): the source -- the sums, a
        denoised or a developed picture -- metered (gain=None) or at the given gain, toned, converted and packed without leaving the
        device: dict(rgba (image_height, image_width, 4) uint8 -- R, G, B and A = 255, written in the chunk's rectangle only, zeros
        elsewhere --, meter (the dict of meter(), None when a gain was given), clip = dict(blown, crushed, nonfinite)).  The bytes are
        those of expose()'s / expose_kat()'s fb on the same picture.  Reads the accumulation, changes nothing of it."""
        p, res = present_config(source, gain, **cfg), B.PresentResult()
        out = np.zeros((image_height, image_width, 4), np.uint8)
        self._ck(B.lib().srt_present(self._h, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_uint8)), 4 * image_width, image_width, image_height, C.byref(res)))
        return dict(rgba=out, meter=_meter_dict(res.meter) if gain is None else None,
                    clip=dict(blown=res.tone.blown, crushed=res.tone.crushed, nonfinite=res.tone.nonfinite))

    def present_kat(self, xyz_mean, gain=None, **cfg):
        """present() on an explicit XYZ-mean image (srt_meter_kat when gain is None, then srt_present_kat): xyz_mean (h, w, 3) float32 ->
        the dict of present() with an (h, w, 4) picture.  Needs no scene and no accumulation."""
        mcfg, tcfg = _split_expose_cfg(cfg)
        img = _xyz_image("present_kat", xyz_mean)
        meter = None
        if gain is None:
            tone_config(gain=1.0, **tcfg)
            meter = self.meter_kat(img, **mcfg)
            gain = meter["gain"]
        elif mcfg:
            raise ValueError("present_kat: %s given with an explicit gain, which is not metered" % ", ".join(sorted(mcfg)))
        t, res = tone_config(gain=gain, **tcfg), B.ToneResult()
        out = np.zeros(img.shape[:2] + (4,), np.uint8)
        self._ck(B.lib().srt_present_kat(self._h, C.byref(t), B.fptr(img), img.shape[1], img.shape[0], out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(res)))
        return dict(rgba=out, meter=meter, clip=dict(blown=res.blown, crushed=res.crushed, nonfinite=res.nonfinite))

    def present_last_ms(self):
        """kernel-only ms of the context's last present kernel (srt_present_last_ms)"""
        ms = C.c_float()
        self._ck(B.lib().srt_present_last_ms(self._h, C.byref(ms)))
        return ms.value

    def _despeckle_cfg(self, who, despeckle, picture=None):
        """srt_despeckle from the keywords of despeckle_config; floor None: the lit pixels' median bin, metered on the accumulation or on
        `picture` (its y_ref at percentile_ppm = 500000; 0 when nothing is metered)"""
        kw = dict(despeckle or {})
        unknown = sorted(set(kw) - set(_DESPECKLE_KEYS))
        if unknown:
            raise TypeError("%s: unknown despeckle keyword(s) %s (%s)" % (who, ", ".join(unknown), ", ".join(_DESPECKLE_KEYS)))
        d = despeckle_config(**kw)          # (a bad value is an error before the device is touched)
        if kw.get("floor") is None:
            m = self.meter(percentile_ppm=500000) if picture is None else self.meter_kat(picture, percentile_ppm=500000)
            d.floor = m["y_ref"]
        return d

    def despeckle(self, image_width, image_height, **cfg):
        """the firefly filter over the context's accumulation, of any kind, on the device (srt_despeckle_accum; cfg: the keywords of
        despeckle_config; floor=None meters first, as expose(gain=None) does): dict(xyz, lin, fb) of (image_height, image_width, 3)
        float32 arrays -- the clamped XYZ mean, its unquantised and its quantised sRGB --, scale (image_height, image_width) -- the
        factor every pixel was multiplied by, 1 where it was kept --, written in the chunk's rectangle only, clip = dict(clamped,
        nonfinite, alone) and floor, the floor used.  Reads the accumulation, changes nothing of it."""
        d, res = self._despeckle_cfg("despeckle", cfg), B.DespeckleResult()
        out = [np.zeros((image_height, image_width, 3), np.float32) for _ in range(3)]
        scale = np.zeros((image_height, image_width), np.float32)
        self._ck(B.lib().srt_despeckle_accum(self._h, C.byref(d), B.fptr(out[0]), B.fptr(out[1]), B.fptr(out[2]), B.fptr(scale), C.byref(res), image_width, image_height))
        return dict(xyz=out[0], lin=out[1], fb=out[2], scale=scale, floor=d.floor, clip=dict(clamped=res.clamped, nonfinite=res.nonfinite, alone=res.alone))

    def despeckle_kat(self, xyz_mean, **cfg):
        """the firefly filter on an explicit XYZ-mean image (srt_meter_kat when floor is None, then srt_despeckle_kat): xyz_mean (h, w, 3)
        float32 -> dict(xyz (h, w, 3), scale (h, w), floor, clip).  Needs no scene and no accumulation."""
        img = _xyz_image("despeckle_kat", xyz_mean)
        d, res = self._despeckle_cfg("despeckle_kat", cfg, img), B.DespeckleResult()
        out, scale = np.zeros(img.shape, np.float32), np.zeros(img.shape[:2], np.float32)
        self._ck(B.lib().srt_despeckle_kat(self._h, C.byref(d), B.fptr(img), img.shape[1], img.shape[0], B.fptr(out), B.fptr(scale), C.byref(res)))
        return dict(xyz=out, scale=scale, floor=d.floor, clip=dict(clamped=res.clamped, nonfinite=res.nonfinite, alone=res.alone))

    def despeckle_last_ms(self):
        """kernel-only ms of the context's last despeckle kernel (srt_despeckle_last_ms)"""
        ms = C.c_float()
        self._ck(B.lib().srt_despeckle_last_ms(self._h, C.byref(ms)))
        return ms.value

    def denoise_despeckled(self, image_width, image_height, despeckle=None, **cfg):
        """denoise() with the firefly filter between the prepass and level 0 (srt_denoise_features_ds; despeckle: a dict of the keywords
        of despeckle_config, None: the defaults; cfg: the keywords of denoise_config): the dict of denoise().  levels=0 returns the
        despeckled mean; floor=inf equals denoise().  Reads the accumulation, changes nothing of it."""
        c = denoise_config(**cfg)
        d = self._despeckle_cfg("denoise_despeckled", despeckle)
        out = [np.zeros((image_height, image_width, 3), np.float32) for _ in range(3)]
        self._ck(B.lib().srt_denoise_features_ds(self._h, C.byref(d), C.byref(c), B.fptr(out[0]), B.fptr(out[1]), B.fptr(out[2]), image_width, image_height))
        return dict(xyz=out[0], lin=out[1], fb=out[2])

    def present_despeckled(self, image_width, image_height, source="accum", gain=None, despeckle=None, **cfg):
        """present() with the firefly filter in front (srt_present_despeckled; source "accum" or "denoise"; despeckle: a dict of the
        keywords of despeckle_config, None: the defaults; the other arguments are present_config's): the dict of present() plus
        despeckle = dict(clamped, nonfinite, alone).  Metering (gain=None) meters the despeckled picture.  Reads the accumulation,
        changes nothing of it."""
        p, res, dres = present_config(source, gain, **cfg), B.PresentResult(), B.DespeckleResult()
        if source not in ("accum", "denoise"):
            raise ValueError("present_despeckled: source must be \"accum\" or \"denoise\", got %r" % (source,))
        d = self._despeckle_cfg("present_despeckled", despeckle)
        out = np.zeros((image_height, image_width, 4), np.uint8)
        self._ck(B.lib().srt_present_despeckled(self._h, C.byref(p), C.byref(d), out.ctypes.data_as(C.POINTER(C.c_uint8)), 4 * image_width, image_width,
                                                image_height, C.byref(res), C.byref(dres)))
        return dict(rgba=out, meter=_meter_dict(res.meter) if gain is None else None,
                    clip=dict(blown=res.tone.blown, crushed=res.tone.crushed, nonfinite=res.tone.nonfinite),
                    despeckle=dict(clamped=dres.clamped, nonfinite=dres.nonfinite, alone=dres.alone))

    def temporal(self, image_width, image_height, **cfg):
        """temporal reprojection of the context's featured accumulation, on the device (srt_temporal_accum; cfg: the keywords of
        temporal_config): the picture blended into the history the previous call left, which survives set_camera and accum_reset*:
        dict(xyz, lin, fb) of (image_height, image_width, 3) float32 arrays -- the blended XYZ mean, its unquantised and its quantised
        sRGB --, len (image_height, image_width) -- the history length behind every pixel, 1 where it is fresh --, motion
        (image_height, image_width, 2) -- where the pixel's surface lay in the previous frame minus where it lies now, in pixels, NaN
        where that is nowhere --, written in the chunk's rectangle only, and stats, the dict of temporal_stats.  Reads the accumulation
        and advances the history; changes nothing else."""
        t, res = _temporal_cfg("temporal", cfg), B.TemporalResult()
        out = [np.zeros((image_height, image_width, 3), np.float32) for _ in range(3)]
        length, motion = np.zeros((image_height, image_width), np.float32), np.zeros((image_height, image_width, 2), np.float32)
        self._ck(B.lib().srt_temporal_accum(self._h, C.byref(t), B.fptr(out[0]), B.fptr(out[1]), B.fptr(out[2]), B.fptr(length), B.fptr(motion), C.byref(res),
                                            image_width, image_height))
        return dict(xyz=out[0], lin=out[1], fb=out[2], len=length, motion=motion, stats=temporal_stats(res))

    def temporal_kat(self, cur_cam, xyz_mean, guides, prev_cam=None, hist_colour=None, hist_guides=None, offx=0, offy=0, **cfg):
        """the temporal kernel on explicit inputs (srt_temporal_kat): xyz_mean (h, w, 3), guides (h, w, 8) = (N, z, A, coverage) of the
        rectangle at image offset (offx, offy) under the camera cur_cam; the history hist_colour (h, w, 4) = (XYZ, len), hist_guides
        (h, w, 8) written under prev_cam -- all three None: no history.  dict(colour (h, w, 4), guides (h, w, 8) -- the new history --,
        motion (h, w, 2), stats).  Needs no scene and no accumulation, and leaves the context's own history alone."""
        t, res = _temporal_cfg("temporal_kat", cfg), B.TemporalResult()
        img = _xyz_image("temporal_kat", xyz_mean)
        g = np.ascontiguousarray(guides, np.float32)
        if g.shape != img.shape[:2] + (8,):
            raise ValueError("temporal_kat: needs guides %r, got %r" % (img.shape[:2] + (8,), g.shape))
        given = [v is not None for v in (prev_cam, hist_colour, hist_guides)]
        if any(given) and not all(given):
            raise ValueError("temporal_kat: a history is prev_cam, hist_colour and hist_guides together")
        hc = hg = None
        if all(given):
            hc, hg = np.ascontiguousarray(hist_colour, np.float32), np.ascontiguousarray(hist_guides, np.float32)
            if hc.shape != img.shape[:2] + (4,) or hg.shape != g.shape:
                raise ValueError("temporal_kat: needs hist_colour %r and hist_guides %r, got %r and %r" % (img.shape[:2] + (4,), g.shape, hc.shape, hg.shape))
        colour, og, motion = np.zeros(img.shape[:2] + (4,), np.float32), np.zeros(g.shape, np.float32), np.zeros(img.shape[:2] + (2,), np.float32)
        self._ck(B.lib().srt_temporal_kat(self._h, C.byref(t), C.byref(cur_cam), C.byref(prev_cam) if all(given) else None, B.fptr(img), B.fptr(g),
                                          B.fptr(hc) if all(given) else None, B.fptr(hg) if all(given) else None, img.shape[1], img.shape[0],
                                          int(offx), int(offy), B.fptr(colour), B.fptr(og), B.fptr(motion), C.byref(res)))
        return dict(colour=colour, guides=og, motion=motion, stats=temporal_stats(res))

    def temporal_reset(self):
        """drop the temporal history: the next temporal call is a first frame (srt_temporal_reset).  upload_scene, init_device_params
        and set_partition drop it too; set_camera and accum_reset* do not."""
        self._ck(B.lib().srt_temporal_reset(self._h))

    def temporal_last_ms(self):
        """kernel-only ms of the context's last temporal kernel (srt_temporal_last_ms)"""
        ms = C.c_float()
        self._ck(B.lib().srt_temporal_last_ms(self._h, C.byref(ms)))
        return ms.value

    def denoise_temporal(self, image_width, image_height, temporal=None, despeckle=None, **cfg):
        """denoise() with the temporal stage between the prepass and level 0 (srt_denoise_features_temporal; temporal: a dict of the
        keywords of temporal_config, None: the defaults; despeckle: a dict of the keywords of despeckle_config -- the firefly filter
        runs in front of the stage --, None: no firefly filter; cfg: the keywords of denoise_config): the dict of denoise() plus stats,
        the dict of temporal_stats.  The history is the stage's output, not the filtered picture, and it is the one temporal() keeps.
        With no history it equals denoise() / denoise_despeckled()."""
        c, t, res = denoise_config(**cfg), _temporal_cfg("denoise_temporal", temporal), B.TemporalResult()
        d = None if despeckle is None else self._despeckle_cfg("denoise_temporal", despeckle)
        out = [np.zeros((image_height, image_width, 3), np.float32) for _ in range(3)]
        self._ck(B.lib().srt_denoise_features_temporal(self._h, C.byref(t), None if d is None else C.byref(d), C.byref(c), B.fptr(out[0]), B.fptr(out[1]),
                                                       B.fptr(out[2]), C.byref(res), image_width, image_height))
        return dict(xyz=out[0], lin=out[1], fb=out[2], stats=temporal_stats(res))

    def present_temporal(self, image_width, image_height, source="accum", gain=None, temporal=None, despeckle=None, **cfg):
        """present() with the temporal stage in front (srt_present_temporal; source "accum" or "denoise", on a featured accumulation;
        temporal and despeckle as denoise_temporal takes them; the other arguments are present_config's): the dict of present() plus
        temporal, the dict of temporal_stats.  Metering (gain=None) meters the stage's output.  Reads the accumulation and advances
        the history."""
        p, res, tres = present_config(source, gain, **cfg), B.PresentResult(), B.TemporalResult()
        if source not in ("accum", "denoise"):
            raise ValueError("present_temporal: source must be \"accum\" or \"denoise\", got %r" % (source,))
        t = _temporal_cfg("present_temporal", temporal)
        d = None if despeckle is None else self._despeckle_cfg("present_temporal", despeckle)
        out = np.zeros((image_height, image_width, 4), np.uint8)
        self._ck(B.lib().srt_present_temporal(self._h, C.byref(p), C.byref(t), None if d is None else C.byref(d), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              4 * image_width, image_width, image_height, C.byref(res), C.byref(tres)))
        return dict(rgba=out, meter=_meter_dict(res.meter) if gain is None else None,
                    clip=dict(blown=res.tone.blown, crushed=res.tone.crushed, nonfinite=res.tone.nonfinite), temporal=temporal_stats(tres))

    # ---- surface motion: the temporal history carried across refits (srt_c_api.h, "Surface motion") ----
    def track_motion(self, on=True):
        """switch motion tracking (srt_temporal_track_motion; off by default): with it on the context keeps the vertices of its scene and
        of its temporal history, a refit KEEPS the history, and the *_moving calls reproject across it.  Switching drops the history and
        leaves the vertices unknown until the next upload_scene or refit."""
        self._ck(B.lib().srt_temporal_track_motion(self._h, 1 if on else 0))

    @property
    def tracking(self):
        """(on, refits_pending) of srt_temporal_tracking: the switch, and the refits since the history was last written"""
        on, n = C.c_int(), C.c_uint32()
        self._ck(B.lib().srt_temporal_tracking(self._h, C.byref(on), C.byref(n)))
        return bool(on.value), n.value

    def surface_motion(self, w, h, ox=0, oy=0):
        """the surface-motion pass on the context's camera, scene and tracked vertices (srt_surface_motion) over the w x h rectangle at
        image offset (ox, oy): dict(point (h, w, 4) float32 -- where the surface point the pixel's centre ray sees lay when the history
        was written, and 1 where that is known --, tri (h, w) int32 -- the triangle, -1 for a miss --, bary (h, w, 3) float32 --
        (t, beta, gamma) --, stats = motion_stats).  Needs tracking on and known vertices; only reads."""
        w, h, ox, oy = _motion_rect("surface_motion", w, h, ox, oy)
        point, tri, bary, res = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.int32), np.zeros((h, w, 3), np.float32), B.MotionResult()
        self._ck(B.lib().srt_surface_motion(self._h, w, h, ox, oy, B.fptr(point), tri.ctypes.data_as(C.POINTER(C.c_int32)), B.fptr(bary), C.byref(res)))
        return dict(point=point, tri=tri, bary=bary, stats=motion_stats(res))

    def surface_motion_kat(self, cam, cur_verts, w, h, ox=0, oy=0, prev_verts=None):
        """the same kernel on the uploaded scene, the camera `cam` and explicit vertex arrays (srt_surface_motion_kat): cur_verts
        (n_tris, 3, 3) float32 MUST be the vertices the uploaded scene was made from (the caller's promise), prev_verts the same
        triangles when the history was written (None: nothing moved).  The dict of surface_motion.  Works with tracking off and
        touches no context state."""
        if not isinstance(cam, B.CameraData):
            raise TypeError("surface_motion_kat: cam is no CameraData (camera_init makes one), got %r" % type(cam).__name__)
        w, h, ox, oy = _motion_rect("surface_motion_kat", w, h, ox, oy)
        cur = refit_vertices("surface_motion_kat: cur_verts", cur_verts)
        prev = None
        if prev_verts is not None:
            prev = refit_vertices("surface_motion_kat: prev_verts", prev_verts)
            if prev.shape != cur.shape:
                raise ValueError("surface_motion_kat: prev_verts %r and cur_verts %r differ in shape" % (prev.shape, cur.shape))
        point, tri, bary, res = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.int32), np.zeros((h, w, 3), np.float32), B.MotionResult()
        self._ck(B.lib().srt_surface_motion_kat(self._h, C.byref(cam), None if prev is None else B.fptr(prev), B.fptr(cur), cur.shape[0], w, h, ox, oy,
                                                B.fptr(point), tri.ctypes.data_as(C.POINTER(C.c_int32)), B.fptr(bary), C.byref(res)))
        return dict(point=point, tri=tri, bary=bary, stats=motion_stats(res))

    def motion_last_ms(self):
        """kernel-only ms of the context's last motion kernel (srt_motion_last_ms)"""
        ms = C.c_float()
        self._ck(B.lib().srt_motion_last_ms(self._h, C.byref(ms)))
        return ms.value

    def temporal_moving(self, image_width, image_height, **cfg):
        """temporal() across refits (srt_temporal_accum_moving): the motion pass on the accumulation's rectangle, then the stage on the
        points it tracked.  The dict of temporal() plus surface, the dict of motion_stats.  Needs tracking on and known vertices."""
        t, res, mres = _temporal_cfg("temporal_moving", cfg), B.TemporalResult(), B.MotionResult()
        out = [np.zeros((image_height, image_width, 3), np.float32) for _ in range(3)]
        length, motion = np.zeros((image_height, image_width), np.float32), np.zeros((image_height, image_width, 2), np.float32)
        self._ck(B.lib().srt_temporal_accum_moving(self._h, C.byref(t), B.fptr(out[0]), B.fptr(out[1]), B.fptr(out[2]), B.fptr(length), B.fptr(motion),
                                                   C.byref(res), image_width, image_height, C.byref(mres)))
        return dict(xyz=out[0], lin=out[1], fb=out[2], len=length, motion=motion, stats=temporal_stats(res), surface=motion_stats(mres))

    def temporal_moving_kat(self, cur_cam, xyz_mean, guides, prev_point, prev_cam=None, hist_colour=None, hist_guides=None, offx=0, offy=0, **cfg):
        """temporal_kat with the tracked points prev_point (h, w, 4) = (Pprev, valid) of surface_motion (srt_temporal_moving_kat): a hit
        pixel projects its tracked point, or has no history where valid is not 1.  The dict of temporal_kat."""
        t, res = _temporal_cfg("temporal_moving_kat", cfg), B.TemporalResult()
        img = _xyz_image("temporal_moving_kat", xyz_mean)
        g = np.ascontiguousarray(guides, np.float32)
        if g.shape != img.shape[:2] + (8,):
            raise ValueError("temporal_moving_kat: needs guides %r, got %r" % (img.shape[:2] + (8,), g.shape))
        pp = np.ascontiguousarray(prev_point, np.float32)
        if pp.shape != img.shape[:2] + (4,):
            raise ValueError("temporal_moving_kat: needs prev_point %r, got %r" % (img.shape[:2] + (4,), pp.shape))
        given = [v is not None for v in (prev_cam, hist_colour, hist_guides)]
        if any(given) and not all(given):
            raise ValueError("temporal_moving_kat: a history is prev_cam, hist_colour and hist_guides together")
        hc = hg = None
        if all(given):
            hc, hg = np.ascontiguousarray(hist_colour, np.float32), np.ascontiguousarray(hist_guides, np.float32)
            if hc.shape != img.shape[:2] + (4,) or hg.shape != g.shape:
                raise ValueError("temporal_moving_kat: needs hist_colour %r and hist_guides %r, got %r and %r" % (img.shape[:2] + (4,), g.shape, hc.shape, hg.shape))
        colour, og, motion = np.zeros(img.shape[:2] + (4,), np.float32), np.zeros(g.shape, np.float32), np.zeros(img.shape[:2] + (2,), np.float32)
        self._ck(B.lib().srt_temporal_moving_kat(self._h, C.byref(t), C.byref(cur_cam), C.byref(prev_cam) if all(given) else None, B.fptr(img), B.fptr(g),
                                                 B.fptr(hc) if all(given) else None, B.fptr(hg) if all(given) else None, img.shape[1], img.shape[0],
                                                 int(offx), int(offy), B.fptr(colour), B.fptr(og), B.fptr(motion), C.byref(res), B.fptr(pp)))
        return dict(colour=colour, guides=og, motion=motion, stats=temporal_stats(res))

    def denoise_temporal_moving(self, image_width, image_height, temporal=None, despeckle=None, **cfg):
        """denoise_temporal across refits (srt_denoise_features_temporal_moving): its dict plus surface, the dict of motion_stats"""
        c, t, res, mres = denoise_config(**cfg), _temporal_cfg("denoise_temporal_moving", temporal), B.TemporalResult(), B.MotionResult()
        d = None if despeckle is None else self._despeckle_cfg("denoise_temporal_moving", despeckle)
        out = [np.zeros((image_height, image_width, 3), np.float32) for _ in range(3)]
        self._ck(B.lib().srt_denoise_features_temporal_moving(self._h, C.byref(t), None if d is None else C.byref(d), C.byref(c), B.fptr(out[0]), B.fptr(out[1]),
                                                              B.fptr(out[2]), C.byref(res), image_width, image_height, C.byref(mres)))
        return dict(xyz=out[0], lin=out[1], fb=out[2], stats=temporal_stats(res), surface=motion_stats(mres))

    def present_temporal_moving(self, image_width, image_height, source="accum", gain=None, temporal=None, despeckle=None, **cfg):
        """present_temporal across refits (srt_present_temporal_moving): its dict plus surface, the dict of motion_stats"""
        p, res, tres, mres = present_config(source, gain, **cfg), B.PresentResult(), B.TemporalResult(), B.MotionResult()
        if source not in ("accum", "denoise"):
            raise ValueError("present_temporal_moving: source must be \"accum\" or \"denoise\", got %r" % (source,))
        t = _temporal_cfg("present_temporal_moving", temporal)
        d = None if despeckle is None else self._despeckle_cfg("present_temporal_moving", despeckle)
        out = np.zeros((image_height, image_width, 4), np.uint8)
        self._ck(B.lib().srt_present_temporal_moving(self._h, C.byref(p), C.byref(t), None if d is None else C.byref(d), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                     4 * image_width, image_width, image_height, C.byref(res), C.byref(tres), C.byref(mres)))
        return dict(rgba=out, meter=_meter_dict(res.meter) if gain is None else None,
                    clip=dict(blown=res.tone.blown, crushed=res.tone.crushed, nonfinite=res.tone.nonfinite), temporal=temporal_stats(tres),
                    surface=motion_stats(mres))

    # ---- variance measured across frames: the moments in the history guide the filter (srt_c_api.h, "Variance measured across frames") ----
    def denoise_temporal_vg(self, image_width, image_height, temporal=None, despeckle=None, min_len=4, moving=False, **vg_cfg):
        """denoise_vg() behind the temporal stage, guided by the variance the history measured (srt_denoise_features_temporal_vg;
        temporal and despeckle as denoise_temporal takes them; min_len and moving: the keywords of temporal_vg_config; vg_cfg: the
        keywords of denoise_vg_config): the stage also carries the first and second luminance moment, and where their own history is at
        least min_len frames long the levels are guided by the variance they measure, elsewhere by the spatial estimate of the stage's
        output.  dict(xyz, lin, fb, var -- var[..., 0] the variance chosen --, stats = temporal_stats, n_temporal -- the pixels that
        took the temporal variance; moving=True: and surface = motion_stats).  The history is the stage's output and the one temporal()
        keeps; a moment-less temporal call in between restarts the moments, not the colour."""
        c, t, v = denoise_vg_config(**vg_cfg), _temporal_cfg("denoise_temporal_vg", temporal), temporal_vg_config(min_len, moving)
        d = None if despeckle is None else self._despeckle_cfg("denoise_temporal_vg", despeckle)
        res, mres, n = B.TemporalResult(), B.MotionResult(), C.c_uint64()
        out = [np.zeros((image_height, image_width, 3), np.float32) for _ in range(3)]
        var = np.zeros((image_height, image_width, 2), np.float32)
        self._ck(B.lib().srt_denoise_features_temporal_vg(self._h, C.byref(t), None if d is None else C.byref(d), C.byref(c), C.byref(v), B.fptr(out[0]),
                                                          B.fptr(out[1]), B.fptr(out[2]), B.fptr(var), C.byref(res), C.byref(n), C.byref(mres), image_width,
                                                          image_height))
        self._moments_image = (image_width, image_height)
        picture = dict(xyz=out[0], lin=out[1], fb=out[2], var=var, stats=temporal_stats(res), n_temporal=n.value)
        if v.moving:
            picture["surface"] = motion_stats(mres)
        return picture

    def present_temporal_vg(self, image_width, image_height, gain=None, temporal=None, despeckle=None, min_len=4, moving=False, **cfg):
        """present() of the chain of denoise_temporal_vg (srt_present_temporal_vg; the source is "denoise_vg", cfg the other keywords of
        present_config): the dict of present_temporal plus n_temporal (moving=True: and surface)."""
        p, res, tres, mres, n = present_config("denoise_vg", gain, **cfg), B.PresentResult(), B.TemporalResult(), B.MotionResult(), C.c_uint64()
        t, v = _temporal_cfg("present_temporal_vg", temporal), temporal_vg_config(min_len, moving)
        d = None if despeckle is None else self._despeckle_cfg("present_temporal_vg", despeckle)
        out = np.zeros((image_height, image_width, 4), np.uint8)
        self._ck(B.lib().srt_present_temporal_vg(self._h, C.byref(p), C.byref(t), None if d is None else C.byref(d), C.byref(v),
                                                 out.ctypes.data_as(C.POINTER(C.c_uint8)), 4 * image_width, image_width, image_height, C.byref(res), C.byref(tres),
                                                 C.byref(n), C.byref(mres)))
        self._moments_image = (image_width, image_height)
        picture = dict(rgba=out, meter=_meter_dict(res.meter) if gain is None else None,
                       clip=dict(blown=res.tone.blown, crushed=res.tone.crushed, nonfinite=res.tone.nonfinite), temporal=temporal_stats(tres),
                       n_temporal=n.value)
        if v.moving:
            picture["surface"] = motion_stats(mres)
        return picture

    def temporal_moments_kat(self, cur_cam, xyz_mean, guides, prev_cam=None, hist_colour=None, hist_guides=None, hist_moments=None, prev_point=None,
                             offx=0, offy=0, **cfg):
        """temporal_kat with the moments (srt_temporal_moments_kat): hist_moments (h, w, 4) = (m1, m2, mlen, 0) of the previous call, None
        for none; prev_point (h, w, 4): the moving stage of temporal_moving_kat, None: the static one.  The dict of temporal_kat plus
        moments (h, w, 4), the new moments history."""
        t, res = _temporal_cfg("temporal_moments_kat", cfg), B.TemporalResult()
        img = _xyz_image("temporal_moments_kat", xyz_mean)
        g = np.ascontiguousarray(guides, np.float32)
        if g.shape != img.shape[:2] + (8,):
            raise ValueError("temporal_moments_kat: needs guides %r, got %r" % (img.shape[:2] + (8,), g.shape))
        given = [v is not None for v in (prev_cam, hist_colour, hist_guides)]
        if any(given) and not all(given):
            raise ValueError("temporal_moments_kat: a history is prev_cam, hist_colour and hist_guides together")
        hc = hg = hm = pp = None
        if all(given):
            hc, hg = np.ascontiguousarray(hist_colour, np.float32), np.ascontiguousarray(hist_guides, np.float32)
            if hc.shape != img.shape[:2] + (4,) or hg.shape != g.shape:
                raise ValueError("temporal_moments_kat: needs hist_colour %r and hist_guides %r, got %r and %r" % (img.shape[:2] + (4,), g.shape, hc.shape, hg.shape))
        for name, v in (("hist_moments", hist_moments), ("prev_point", prev_point)):
            if v is not None and np.shape(v) != img.shape[:2] + (4,):
                raise ValueError("temporal_moments_kat: needs %s %r, got %r" % (name, img.shape[:2] + (4,), np.shape(v)))
        if hist_moments is not None:
            if not all(given):
                raise ValueError("temporal_moments_kat: hist_moments given without a colour history")
            hm = np.ascontiguousarray(hist_moments, np.float32)
        if prev_point is not None:
            pp = np.ascontiguousarray(prev_point, np.float32)
        colour, og, motion = np.zeros(img.shape[:2] + (4,), np.float32), np.zeros(g.shape, np.float32), np.zeros(img.shape[:2] + (2,), np.float32)
        moments = np.zeros(img.shape[:2] + (4,), np.float32)
        self._ck(B.lib().srt_temporal_moments_kat(self._h, C.byref(t), C.byref(cur_cam), C.byref(prev_cam) if all(given) else None, B.fptr(img), B.fptr(g),
                                                  B.fptr(hc) if all(given) else None, B.fptr(hg) if all(given) else None, img.shape[1], img.shape[0],
                                                  int(offx), int(offy), B.fptr(colour), B.fptr(og), B.fptr(motion), C.byref(res),
                                                  None if pp is None else B.fptr(pp), None if hm is None else B.fptr(hm), B.fptr(moments)))
        return dict(colour=colour, guides=og, motion=motion, moments=moments, stats=temporal_stats(res))

    def temporal_variance_kat(self, moments, length, spatial_var, min_len=4):
        """the choice of the variance on explicit inputs (srt_temporal_variance_kat): moments (h, w, 4) and length (h, w) as the stage
        left them, spatial_var (h, w) the spatial estimate -> (var (h, w) float32, n_temporal): the moments' variance of the mean,
        (m2 - m1^2) / len, where the moments are at least min_len frames long, spatial_var elsewhere, and the number of the former."""
        v = temporal_vg_config(min_len)
        m = np.ascontiguousarray(moments, np.float32)
        if m.ndim != 3 or m.shape[2] != 4 or m.shape[0] == 0 or m.shape[1] == 0:
            raise ValueError("temporal_variance_kat: needs moments (h, w, 4), got %r" % (m.shape,))
        ln, vs = np.ascontiguousarray(length, np.float32), np.ascontiguousarray(spatial_var, np.float32)
        if ln.shape != m.shape[:2] or vs.shape != m.shape[:2]:
            raise ValueError("temporal_variance_kat: needs length and spatial_var %r, got %r and %r" % (m.shape[:2], ln.shape, vs.shape))
        out, n = np.zeros(m.shape[:2], np.float32), C.c_uint64()
        self._ck(B.lib().srt_temporal_variance_kat(self._h, B.fptr(m), B.fptr(ln), B.fptr(vs), v.min_len, m.shape[1], m.shape[0], B.fptr(out), C.byref(n)))
        return out, n.value

    def temporal_moments(self, image_width=None, image_height=None):
        """the context's current moments history (srt_read_temporal_moments): (image_height, image_width, 4) float32 = (m1, m2, mlen, 0),
        written in the history's rectangle only; without arguments the image of this renderer's last denoise_temporal_vg /
        present_temporal_vg.  SrtError when the context holds none (no moments call since the history began, or a moment-less
        temporal call since)."""
        if image_width is None or image_height is None:
            if getattr(self, "_moments_image", None) is None:
                raise ValueError("temporal_moments: no image size given and no denoise_temporal_vg / present_temporal_vg call to take it from")
            image_width, image_height = self._moments_image
        out = np.zeros((image_height, image_width, 4), np.float32)
        self._ck(B.lib().srt_read_temporal_moments(self._h, B.fptr(out), image_width, image_height))
        return out

    def temporal_variance_last_ms(self):
        """kernel-only ms of the context's last choice kernel (srt_temporal_variance_last_ms)"""
        ms = C.c_float()
        self._ck(B.lib().srt_temporal_variance_last_ms(self._h, C.byref(ms)))
        return ms.value

    def accum_reset_features(self):
        """start a FEATURED accumulation (srt_c_api.h): like accum_reset, and each later pass also adds, at the first hit of every
        sample's camera ray, the face-forwarded normal, the hit material's colour, the distance and 1 to the pixel's eight raw float32
        sums (read_features; feature_means normalises them).  Never streamed; accum_reset_adaptive_features is the adaptive one,
        accum_reset_spectral_features the one with a film."""
        self._ck(B.lib().srt_accum_reset_features(self._h))

    def accum_reset_adaptive_features(self, rel_tol, abs_tol=0.0, min_spp=16):
        """start an ADAPTIVE FEATURED accumulation (srt_c_api.h): accum_reset_adaptive with the feature rows of accum_reset_features.
        Image, sums, S2, sample map and RNG state are accum_reset_adaptive's bit for bit; a pixel that stopped after n samples holds the
        feature row of a plain featured n-spp frame.  accum_active, accum_stats and read_features all work on it, and denoise,
        denoise_vg and denoise_mv take it (each pixel normalised by its own count)."""
        self._ck(B.lib().srt_accum_reset_adaptive_features(self._h, C.byref(adaptive_config(rel_tol, abs_tol, min_spp))))

    def accum_reset_spectral_features(self):
        """start a SPECTRAL FEATURED accumulation (srt_c_api.h): accum_reset_spectral with the feature rows of accum_reset_features.
        Image, sums, RNG state and film are accum_reset_spectral's bit for bit, the rows accum_reset_features'.  read_spectral,
        develop_spectral, read_features, denoise and denoise_vg all work on it, and denoise_developed needs it.  Never adaptive:
        accum_reset_adaptive_spectral_features is the adaptive one."""
        self._ck(B.lib().srt_accum_reset_spectral_features(self._h))

    def accum_reset_adaptive_spectral(self, rel_tol, abs_tol=0.0, min_spp=16):
        """start an ADAPTIVE SPECTRAL accumulation (srt_c_api.h): accum_reset_adaptive (same arguments, same stopping rule) with the film of
        accum_reset_spectral.  Image, sums, sample map, active counts and RNG state are accum_reset_adaptive's bit for bit; a pixel's film
        row belongs to the samples that pixel holds (spectral_radiance(film, samples map)), and a converged pixel's row is never touched
        again.  accum_active, accum_stats, read_spectral and develop_spectral take it; develop_spectral_srgb divides a pixel by its own count."""
        self._ck(B.lib().srt_accum_reset_adaptive_spectral(self._h, C.byref(adaptive_config(rel_tol, abs_tol, min_spp))))

    def accum_reset_adaptive_spectral_features(self, rel_tol, abs_tol=0.0, min_spp=16):
        """start an ADAPTIVE SPECTRAL FEATURED accumulation (srt_c_api.h): accum_reset_adaptive_spectral with the feature rows of
        accum_reset_adaptive_features, which they equal bit for bit.  read_features, denoise, denoise_vg and denoise_mv take it as they
        take accum_reset_adaptive_features', and denoise_developed divides colour, guides and developed planes of a pixel by its own count."""
        self._ck(B.lib().srt_accum_reset_adaptive_spectral_features(self._h, C.byref(adaptive_config(rel_tol, abs_tol, min_spp))))

    def read_features(self, image_width, image_height):
        """raw first-hit sums of the featured accumulation's chunk, float32: dict(normal (H, W, 3), albedo (H, W, 3), distance (H, W),
        hits (H, W)); only the chunk's rectangle is written (zeros elsewhere, and at pixels of other ranks)"""
        out = np.zeros((image_height, image_width, FEATURE_CHANNELS), np.float32)
        self._ck(B.lib().srt_read_features(self._h, B.fptr(out), image_width, image_height))
        return split_features(out)

    def denoise(self, image_width, image_height, **cfg):
        """the a-trous denoiser over the context's featured accumulation (srt_denoise_features; cfg: the keywords of denoise_config):
        dict(xyz, lin, fb) of (image_height, image_width, 3) float32 arrays -- the filtered XYZ mean, its unquantised and its quantised
        sRGB -- written in the chunk's rectangle only (the placement of read_features), zeros elsewhere.  Reads the accumulation,
        changes nothing of it."""
        c = denoise_config(**cfg)
        out = [np.zeros((image_height, image_width, 3), np.float32) for _ in range(3)]
        self._ck(B.lib().srt_denoise_features(self._h, C.byref(c), B.fptr(out[0]), B.fptr(out[1]), B.fptr(out[2]), image_width, image_height))
        return dict(xyz=out[0], lin=out[1], fb=out[2])

    def denoise_kat(self, xyz_sums, features, samples, **cfg):
        """the denoiser's device path on explicit inputs (srt_denoise_kat): xyz_sums (h, w, 3) and features (h, w, 8) raw float32 sums
        of `samples` samples -> the filtered XYZ mean (h, w, 3).  Needs no scene and no accumulation."""
        c = denoise_config(**cfg)
        sums = np.ascontiguousarray(xyz_sums, np.float32)
        rows = np.ascontiguousarray(features, np.float32)
        if sums.ndim != 3 or sums.shape[2] != 3 or rows.shape != sums.shape[:2] + (FEATURE_CHANNELS,):
            raise ValueError("denoise_kat: needs xyz_sums (h, w, 3) and features (h, w, %d), got %r and %r" % (FEATURE_CHANNELS, sums.shape, rows.shape))
        out = np.zeros(sums.shape, np.float32)
        self._ck(B.lib().srt_denoise_kat(self._h, C.byref(c), B.fptr(sums), B.fptr(rows), int(samples), sums.shape[1], sums.shape[0], B.fptr(out)))
        return out

    def denoise_developed(self, image_width, image_height, response, scale=1.0, filter=None, **cfg):
        """the film of the context's SPECTRAL FEATURED accumulation developed and denoised on the device (srt_denoise_developed; response,
        scale and filter as develop_spectral, cfg: the keywords of denoise_config): dict(dev (image_height, image_width, K), xyz
        (image_height, image_width, 3)) float32 -- the K developed planes as per-sample means, filtered with the weights the plain
        filter forms from the XYZ colour and the guides, and the filtered XYZ mean, which is denoise()'s xyz bit for bit.  Written in the
        chunk's rectangle only, zeros elsewhere.  Reads the accumulation, changes nothing of it."""
        resp = sensor_response(response, filter)
        s = _develop_scale(scale)
        c = denoise_config(**cfg)
        dev = np.zeros((image_height, image_width, resp.shape[0]), np.float32)
        xyz = np.zeros((image_height, image_width, 3), np.float32)
        self._ck(B.lib().srt_denoise_developed(self._h, C.byref(c), B.fptr(resp), resp.shape[0], s, B.fptr(dev), B.fptr(xyz), image_width, image_height))
        return dict(dev=dev, xyz=xyz)

    def denoise_developed_kat(self, xyz_sums, features, developed, samples, **cfg):
        """the payload denoiser's device path on explicit inputs (srt_denoise_developed_kat): xyz_sums (h, w, 3), features (h, w, 8) and
        developed (h, w, K), 1 <= K <= 16, raw float32 sums of `samples` samples -> (the filtered developed mean (h, w, K), the filtered
        XYZ mean (h, w, 3)).  Needs no scene and no accumulation.  The shapes are checked here (ValueError)."""
        c = denoise_config(**cfg)
        sums = np.ascontiguousarray(xyz_sums, np.float32)
        rows = np.ascontiguousarray(features, np.float32)
        planes = np.ascontiguousarray(developed, np.float32)
        if sums.ndim != 3 or sums.shape[2] != 3 or rows.shape != sums.shape[:2] + (FEATURE_CHANNELS,):
            raise ValueError("denoise_developed_kat: needs xyz_sums (h, w, 3) and features (h, w, %d), got %r and %r" % (FEATURE_CHANNELS, sums.shape, rows.shape))
        if planes.ndim != 3 or planes.shape[:2] != sums.shape[:2] or not 1 <= planes.shape[2] <= MAX_DEVELOP_CHANNELS:
            raise ValueError("denoise_developed_kat: needs developed (h, w, K) with 1 <= K <= %d over the same pixels, got %r" % (MAX_DEVELOP_CHANNELS, planes.shape))
        if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or not 1 <= samples <= 0xffffffff:
            raise ValueError("denoise_developed_kat: samples must be a whole number >= 1, got %r" % (samples,))
        dev = np.zeros(planes.shape, np.float32)
        xyz = np.zeros(sums.shape, np.float32)
        self._ck(B.lib().srt_denoise_developed_kat(self._h, C.byref(c), B.fptr(sums), B.fptr(rows), B.fptr(planes), planes.shape[2], int(samples),
                                                   sums.shape[1], sums.shape[0], B.fptr(dev), B.fptr(xyz)))
        return dev, xyz

    def denoise_developed_counts_kat(self, xyz_sums, features, developed, samples, **cfg):
        """denoise_developed_kat with a per-pixel sample map (srt_denoise_developed_counts_kat): samples (h, w) whole numbers >= 1, the
        count each pixel's sums hold -- the kernels an adaptive spectral featured accumulation runs.  Shapes and map are checked here
        (ValueError)."""
        c = denoise_config(**cfg)
        sums = np.ascontiguousarray(xyz_sums, np.float32)
        rows = np.ascontiguousarray(features, np.float32)
        planes = np.ascontiguousarray(developed, np.float32)
        if sums.ndim != 3 or sums.shape[2] != 3 or rows.shape != sums.shape[:2] + (FEATURE_CHANNELS,):
            raise ValueError("denoise_developed_counts_kat: needs xyz_sums (h, w, 3) and features (h, w, %d), got %r and %r" % (FEATURE_CHANNELS, sums.shape, rows.shape))
        if planes.ndim != 3 or planes.shape[:2] != sums.shape[:2] or not 1 <= planes.shape[2] <= MAX_DEVELOP_CHANNELS:
            raise ValueError("denoise_developed_counts_kat: needs developed (h, w, K) with 1 <= K <= %d over the same pixels, got %r" % (MAX_DEVELOP_CHANNELS, planes.shape))
        raw = np.asarray(samples)
        if raw.dtype == np.bool_ or not np.issubdtype(raw.dtype, np.integer) or raw.shape != sums.shape[:2]:
            raise ValueError("denoise_developed_counts_kat: samples must be whole numbers of shape %r, got %s %r" % (sums.shape[:2], raw.dtype, raw.shape))
        if raw.size and (int(raw.min()) < 1 or int(raw.max()) > 0x7fffffff):
            raise ValueError("denoise_developed_counts_kat: every pixel must hold between 1 and 2^31 - 1 samples")
        counts = np.ascontiguousarray(raw, np.uint32)
        dev = np.zeros(planes.shape, np.float32)
        xyz = np.zeros(sums.shape, np.float32)
        self._ck(B.lib().srt_denoise_developed_counts_kat(self._h, C.byref(c), B.fptr(sums), B.fptr(rows), B.fptr(planes), planes.shape[2],
                                                          counts.ctypes.data_as(C.POINTER(C.c_uint32)), sums.shape[1], sums.shape[0], B.fptr(dev), B.fptr(xyz)))
        return dev, xyz

    def denoise_last_ms(self):
        """kernel-only ms of the last denoise on this context (srt_denoise_last_ms): dict(prepass, levels=[ms per level], epilogue)"""
        pre, epi, n = C.c_float(), C.c_float(), C.c_uint32()
        lv = (C.c_float * 8)()
        self._ck(B.lib().srt_denoise_last_ms(self._h, C.byref(pre), lv, C.byref(epi), C.byref(n)))
        return dict(prepass=pre.value, levels=[lv[i] for i in range(n.value)], epilogue=epi.value)

    def denoise_vg(self, image_width, image_height, **cfg):
        """the variance-guided denoiser over the context's featured accumulation (srt_denoise_features_vg; cfg: the keywords of
        denoise_vg_config): dict(xyz, lin, fb, var) -- the three (image_height, image_width, 3) arrays of denoise and var
        (image_height, image_width, 2): the estimator's variance of Y and the variance after the last level.  Placement as denoise."""
        c = denoise_vg_config(**cfg)
        out = [np.zeros((image_height, image_width, 3), np.float32) for _ in range(3)]
        var = np.zeros((image_height, image_width, 2), np.float32)
        self._ck(B.lib().srt_denoise_features_vg(self._h, C.byref(c), B.fptr(out[0]), B.fptr(out[1]), B.fptr(out[2]), B.fptr(var), image_width, image_height))
        return dict(xyz=out[0], lin=out[1], fb=out[2], var=var)

    def denoise_vg_kat(self, xyz_sums, features, samples, **cfg):
        """the variance-guided denoiser's device path on explicit inputs (srt_denoise_vg_kat; the inputs of denoise_kat) -> (the
        filtered XYZ mean (h, w, 3), var (h, w, 2))"""
        c = denoise_vg_config(**cfg)
        sums = np.ascontiguousarray(xyz_sums, np.float32)
        rows = np.ascontiguousarray(features, np.float32)
        if sums.ndim != 3 or sums.shape[2] != 3 or rows.shape != sums.shape[:2] + (FEATURE_CHANNELS,):
            raise ValueError("denoise_vg_kat: needs xyz_sums (h, w, 3) and features (h, w, %d), got %r and %r" % (FEATURE_CHANNELS, sums.shape, rows.shape))
        out = np.zeros(sums.shape, np.float32)
        var = np.zeros(sums.shape[:2] + (2,), np.float32)
        self._ck(B.lib().srt_denoise_vg_kat(self._h, C.byref(c), B.fptr(sums), B.fptr(rows), int(samples), sums.shape[1], sums.shape[0], B.fptr(out), B.fptr(var)))
        return out, var

    def denoise_mv(self, image_width, image_height, **cfg):
        """the measured-variance denoiser over the context's ADAPTIVE FEATURED accumulation of at least 2 samples
        (srt_denoise_features_mv; cfg: the keywords of denoise_vg_config): the dict of denoise_vg, var[..., 0] being the variance of the
        pixel's mean luminance the sampler measured -- max(S2 / n - (S1 / n)^2, 0) / (n - 1) from the pixel's own count, Y sum and S2 --
        in the place of the spatial estimate."""
        c = denoise_vg_config(**cfg)
        out = [np.zeros((image_height, image_width, 3), np.float32) for _ in range(3)]
        var = np.zeros((image_height, image_width, 2), np.float32)
        self._ck(B.lib().srt_denoise_features_mv(self._h, C.byref(c), B.fptr(out[0]), B.fptr(out[1]), B.fptr(out[2]), B.fptr(var), image_width, image_height))
        return dict(xyz=out[0], lin=out[1], fb=out[2], var=var)

    def denoise_mv_kat(self, xyz_sums, features, samples, sum_y2, **cfg):
        """the measured-variance denoiser's device path on explicit inputs (srt_denoise_mv_kat): xyz_sums (h, w, 3), features (h, w, 8),
        samples (h, w) whole numbers >= 1 -- every pixel's own count -- and sum_y2 (h, w) -> (the filtered XYZ mean (h, w, 3), var
        (h, w, 2)).  Checked here as the library checks it (ValueError): the shapes, and no zero in samples."""
        c = denoise_vg_config(**cfg)
        sums = np.ascontiguousarray(xyz_sums, np.float32)
        rows = np.ascontiguousarray(features, np.float32)
        if sums.ndim != 3 or sums.shape[2] != 3 or rows.shape != sums.shape[:2] + (FEATURE_CHANNELS,):
            raise ValueError("denoise_mv_kat: needs xyz_sums (h, w, 3) and features (h, w, %d), got %r and %r" % (FEATURE_CHANNELS, sums.shape, rows.shape))
        n_in = np.asarray(samples)
        s2 = np.ascontiguousarray(sum_y2, np.float32)
        if n_in.shape != sums.shape[:2] or s2.shape != sums.shape[:2]:
            raise ValueError("denoise_mv_kat: samples and sum_y2 must be (h, w) = %r, got %r and %r" % (sums.shape[:2], n_in.shape, s2.shape))
        if n_in.dtype.kind not in "iu" or (n_in < 1).any() or (n_in > 0x7fffffff).any():
            raise ValueError("denoise_mv_kat: samples must be whole numbers in [1, 2^31 - 1] (every pixel holds at least one sample)")
        n = np.ascontiguousarray(n_in, np.uint32)
        out = np.zeros(sums.shape, np.float32)
        var = np.zeros(sums.shape[:2] + (2,), np.float32)
        self._ck(B.lib().srt_denoise_mv_kat(self._h, C.byref(c), B.fptr(sums), B.fptr(rows), n.ctypes.data_as(C.POINTER(C.c_uint32)), B.fptr(s2),
                                            sums.shape[1], sums.shape[0], B.fptr(out), B.fptr(var)))
        return out, var

    def denoise_estimate_last_ms(self):
        """kernel-only ms of the variance estimator of the last denoise on this context, which must have been variance-guided
        (srt_denoise_estimate_last_ms)"""
        ms = C.c_float()
        self._ck(B.lib().srt_denoise_estimate_last_ms(self._h, C.byref(ms)))
        return ms.value

    def accum_reset_streams(self, k):
        """start a STREAMED accumulation (srt_c_api.h): every pixel has k independent RNG streams (1 <= k <= MAX_STREAMS), stream j of lane
        idx seeded XORWOW(seed + j * n_lanes + idx); a pass of spp_add samples (a multiple of k) draws spp_add / k from every stream, and
        the pixel's XYZ sum is ((S_0 + S_1) + ..) + S_{k-1}, S_j the sum of a plain accumulation of a context seeded seed + j * n_lanes"""
        self._ck(B.lib().srt_accum_reset_streams(self._h, int(k)))

    @property
    def accum_streams(self):
        """the streams per pixel of a streamed accumulation; 0 when the accumulation is not streamed (or there is none)"""
        n = C.c_uint32()
        self._ck(B.lib().srt_accum_streams(self._h, C.byref(n)))
        return n.value

    def set_gather_planes(self, planes):
        """3 (default): the exchange unit is the quantised framebuffer; 9: + the parity planes (unquantised sRGB, XYZ sums)"""
        self._ck(B.lib().srt_set_gather_planes(self._h, planes))
        self.gather_planes = planes

    def tile_buffer(self):
        ptr, n, tl, tp = C.c_void_p(), C.c_size_t(), C.c_uint32(), C.c_uint32()
        self._ck(B.lib().srt_tile_buffer(self._h, C.byref(ptr), C.byref(n), C.byref(tl), C.byref(tp)))
        return ptr.value, n.value, tl.value, tp.value

    def copy_tile_buffer(self, dst_ptr, stream=None):
        self._ck(B.lib().srt_copy_tile_buffer(self._h, C.c_void_p(dst_ptr), C.c_void_p(stream or 0)))

    def scatter_tiles(self, gathered_ptr=None, stream=None):
        self._ck(B.lib().srt_scatter_tiles(self._h, C.c_void_p(gathered_ptr or 0), C.c_void_p(stream or 0)))

    def accum_exchange_size(self, parts=None):
        """floats of this context's accumulation exchange unit for `parts` (gather_parts: names, a mask or None; srt_accum_exchange_size)"""
        n = C.c_size_t()
        self._ck(B.lib().srt_accum_exchange_size(self._h, gather_parts(parts), C.byref(n)))
        return n.value

    def pack_accum(self, dst_ptr, parts=None, hip_stream=None):
        """this rank's own tile records out of the accumulation buffers into device memory at dst_ptr (accum_exchange_size floats);
        asynchronous on the stream `hip_stream`, a handle as render_chunk_accum's `stream` (srt_pack_accum)"""
        self._ck(B.lib().srt_pack_accum(self._h, gather_parts(parts), C.c_void_p(dst_ptr or 0), C.c_void_p(hip_stream or 0)))

    def unpack_accum(self, gathered_ptr, parts=None, hip_stream=None):
        """`world` units, rank-major, in device memory at gathered_ptr into this context's accumulation buffers, for every tile it does not
        own: it then holds what a partition (0, 1) context would hold, until its next pass (srt_unpack_accum)"""
        self._ck(B.lib().srt_unpack_accum(self._h, gather_parts(parts), C.c_void_p(gathered_ptr or 0), C.c_void_p(hip_stream or 0)))

    def accum_gathered(self):
        """the SRT_GATHER_* mask the last unpack_accum since the last pass brought (0: nothing)"""
        m = C.c_uint32()
        self._ck(B.lib().srt_accum_gathered(self._h, C.byref(m)))
        return m.value

    def accum_whole(self, parts=None):
        """True when the context holds the whole chunk for a stage that reads `parts` (gather_parts; the sums, and the counts of an adaptive
        accumulation, are implied): its partition is (0, 1), or the last unpack_accum since its last pass brought all of it
        (srt_accum_whole)"""
        w = C.c_int()
        self._ck(B.lib().srt_accum_whole(self._h, gather_parts(parts), C.byref(w)))
        return bool(w.value)

    def gather_last_ms(self):
        """(pack_ms, unpack_ms) of the context's last pack and unpack kernels, 0 where there was none"""
        a, b = C.c_float(), C.c_float()
        self._ck(B.lib().srt_gather_last_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def dev_fb(self):
        r, g, b, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        self._ck(B.lib().srt_dev_fb(self._h, C.byref(r), C.byref(g), C.byref(b), C.byref(n)))
        return r.value, g.value, b.value, n.value

    def read_fb(self):
        n = self.geom["n_lanes"]
        r, g, b = (np.zeros(n, np.float32) for _ in range(3))
        self._ck(B.lib().srt_read_fb(self._h, B.fptr(r), B.fptr(g), B.fptr(b)))
        return r, g, b

    def read_fb_aux(self, which):
        n = self.geom["n_lanes"]
        r, g, b = (np.zeros(n, np.float32) for _ in range(3))
        self._ck(B.lib().srt_read_fb_aux(self._h, which, B.fptr(r), B.fptr(g), B.fptr(b)))
        return r, g, b

    def read_fb_rowmajor(self, image_width, image_height, into=None):
        if into is None:
            into = tuple(np.zeros(image_width * image_height, np.float32) for _ in range(3))
        r, g, b = into
        self._ck(B.lib().srt_read_fb_rowmajor(self._h, B.fptr(r), B.fptr(g), B.fptr(b), image_width, image_height))
        return r, g, b

    def tile_costs(self, with_max_pixel=False):
        """the cost probe's node visits per local tile; with_max_pixel: (per tile, of each tile's most expensive pixel)"""
        _, _, tl, _ = self.tile_buffer()
        out = np.zeros(tl * (2 if with_max_pixel else 1), np.uint32)
        self._ck(B.lib().srt_get_tile_costs(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return (out[:tl], out[tl:]) if with_max_pixel else out

    def order_children_by_profile(self, scene, width, height, spp, bounce_limit, min_samples=4):
        """re-order the children of `scene`'s tree from one instrumented probe frame of this context's camera (srt_c_api.h); the
        scene is left uploaded; returns the number of nodes whose children were swapped.  init_device_params comes next."""
        n = C.c_uint32(0)
        self._ck(B.lib().srt_order_children_by_profile(self._h, scene.handle, width, height, spp, bounce_limit, min_samples, C.byref(n)))
        return n.value

    def collect_ray_segments(self, width, height, spp, bounce_limit, stride=1, seed=0, capacity=None):
        """a sample of the closest-hit queries of one instrumented frame of this context's camera and uploaded scene
        (srt_collect_ray_segments): (segments (n, 7) float32 -- origin, direction, t_end --, queries that took a ticket).  capacity: the
        most segments to return (default: every one the frame can sample).  init_device_params comes next."""
        if capacity is None:
            capacity = width * height * spp * max(bounce_limit, 1) // max(stride, 1) + 1
        out = np.zeros((capacity, 7), np.float32)
        n, q = C.c_size_t(0), C.c_uint64(0)
        self._ck(B.lib().srt_collect_ray_segments(self._h, width, height, spp, bounce_limit, stride, seed, B.fptr(out), capacity, C.byref(n), C.byref(q)))
        return out[:n.value].copy(), q.value

    def stats(self):
        st = B.Stats()
        self._ck(B.lib().srt_get_stats(self._h, C.byref(st)))
        d = {k: getattr(st, k) for k in ("rays", "paths", "node_visits", "tri_tests", "box_tests")}
        d["util"] = list(st.util)
        d["shade"] = list(st.shade)
        d["waves"] = list(st.waves)
        d["hits"] = st.hits
        d["max_pixel_node_visits"], d["max_pixel_rays"] = st.reserved[0], st.reserved[1]
        return d

    def wave_debug(self):
        """per persistent wave of the last INSTRUMENTED launch: [life, queue-dry time (256-cycle units), rays, rays of its most expensive pixel]"""
        n = int(self.stats()["waves"][0])
        out = np.zeros((n, 4), np.uint32)
        if n:
            self._ck(B.lib().srt_get_wave_debug(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return out

    def last_kernel_ms(self):
        ms = C.c_float()
        self._ck(B.lib().srt_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def calibrate(self, kind, waves_per_simd=4, iters=20000):
        """Issue-rate microkernel (csrc/srt_calib.hip): one workgroup of waves_per_simd * 256 threads on every CU.

        The SIMD's arbiter prefers older waves, so with four resident waves two of them run at their single-wave speed and
        finish at about half of the launch; the rate a SIMD sustains is therefore the instructions of ALL its waves over the
        cycles of the LAST one (wave_cycles_max, = wall x clock), not over the mean wave life -- the mean-based figure of round 2
        (0.585 / cycle) belongs to no SIMD.  `instr_per_cycle_per_simd` is the max-based rate; min / mean / max are all returned."""
        cal = B.Calibration()
        self._ck(B.lib().srt_calibrate(self._h, kind, waves_per_simd, iters, C.byref(cal)))
        n_simd = cal.n_cu * 4
        total = cal.instr_per_wave * cal.n_waves
        clock_ghz = cal.wave_cycles_max / (cal.wall_ms * 1e-3) / 1e9        # the slowest wave spans the launch: its cycles / wall
        return dict(kind=kind, waves_per_simd=cal.waves_per_simd, n_cu=cal.n_cu, wave_cycles_min=cal.wave_cycles_min,
                    wave_cycles_mean=cal.wave_cycles_mean, wave_cycles_max=cal.wave_cycles_max, wall_ms=cal.wall_ms,
                    instr_per_wave=cal.instr_per_wave,
                    instr_per_cycle_per_simd=cal.instr_per_wave * cal.waves_per_simd / cal.wave_cycles_max,
                    instr_per_cycle_per_simd_mean_wave=cal.instr_per_wave * cal.waves_per_simd / cal.wave_cycles_mean,
                    instr_per_s=total / (cal.wall_ms * 1e-3), clock_ghz=clock_ghz, n_simd=n_simd)

    def trace_rays(self, rays):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((rays.shape[0], 4), np.float32)
        self._ck(B.lib().srt_trace_rays(self._h, B.fptr(rays), rays.shape[0], B.fptr(out)))
        return out

    def _query_rays(self, who, rays):
        """('host', float32 (n, 8) C-contiguous array) or ('dev', tensor) for the query entries; every check before the device is touched"""
        if isinstance(rays, np.ndarray):
            if rays.dtype != np.float32:
                raise TypeError("%s: the rays must be float32, got %s" % (who, rays.dtype))
            if rays.ndim != 2 or rays.shape[1] != 8:
                raise ValueError("%s: the rays must have shape (n, 8) -- ox oy oz tmin dx dy dz tmax --, got %r" % (who, rays.shape))
            if rays.shape[0] > B.QUERY_MAX_RAYS:
                raise ValueError("%s: %d rays do not fit the ray counter (at most %d)" % (who, rays.shape[0], B.QUERY_MAX_RAYS))
            return "host", np.ascontiguousarray(rays)
        t = rays
        if not all(hasattr(t, a) for a in ("data_ptr", "is_contiguous", "device", "dtype", "shape")):
            raise TypeError("%s: the rays must be a numpy array or a torch tensor (n, 8) float32, got %r" % (who, type(t).__name__))
        import torch
        if t.dtype != torch.float32:
            raise TypeError("%s: the tensor must be float32, got %s" % (who, t.dtype))
        if t.dim() != 2 or t.shape[1] != 8:
            raise ValueError("%s: the tensor must have shape (n, 8) -- ox oy oz tmin dx dy dz tmax --, got %r" % (who, tuple(t.shape)))
        if t.shape[0] > B.QUERY_MAX_RAYS:
            raise ValueError("%s: %d rays do not fit the ray counter (at most %d)" % (who, t.shape[0], B.QUERY_MAX_RAYS))
        if not t.is_contiguous():
            raise ValueError("%s: the tensor must be contiguous" % who)
        if t.shape[0] > 0 and t.data_ptr() % 16:
            raise ValueError("%s: the tensor's data must be 16-byte aligned (a row is two 16-byte loads)" % who)
        if t.device.type != "cuda" or (t.device.index if t.device.index is not None else torch.cuda.current_device()) != self.device:
            raise ValueError("%s: the tensor lives on %s, the renderer on GPU %d" % (who, t.device, self.device))
        return "dev", t

    def intersect(self, rays):
        """closest hits over each ray's interval (srt_intersect_rays / srt_intersect_rays_dev): rays (n, 8) float32 rows ox oy oz tmin dx dy dz
        tmax (ray_batch makes them).  A numpy array goes through the host entry and gives numpy (n, 4) float32 rows in trace_rays' layout --
        t (0 on a miss), tri or -1, front_face, mat_index.  A contiguous, 16-byte aligned float32 CUDA tensor on this renderer's device goes
        through the device entry on torch.cuda.current_stream(), without a host synchronisation, and gives a tensor."""
        kind, r = self._query_rays("Renderer.intersect", rays)
        if kind == "host":
            out = np.zeros((r.shape[0], 4), np.float32)
            self._ck(B.lib().srt_intersect_rays(self._h, B.fptr(r), r.shape[0], B.fptr(out)))
            return out
        import torch
        out = torch.empty((r.shape[0], 4), dtype=torch.float32, device=r.device)
        stream = torch.cuda.current_stream(r.device).cuda_stream
        self._ck(B.lib().srt_intersect_rays_dev(self._h, C.c_void_p(r.data_ptr()), r.shape[0], C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def occluded(self, rays):
        """any-hit occlusion over each ray's interval (srt_occluded_rays / srt_occluded_rays_dev): True where [tmin, tmax] holds a hit.  The
        rays and the two paths as in intersect; the answer is a bool numpy array or a bool tensor of n entries."""
        kind, r = self._query_rays("Renderer.occluded", rays)
        if kind == "host":
            out = np.zeros(r.shape[0], np.uint8)
            self._ck(B.lib().srt_occluded_rays(self._h, B.fptr(r), r.shape[0], out.ctypes.data_as(C.POINTER(C.c_uint8))))
            return out.astype(bool)
        import torch
        out = torch.empty(r.shape[0], dtype=torch.bool, device=r.device)      # (one byte per entry: the kernel writes 0 / 1)
        stream = torch.cuda.current_stream(r.device).cuda_stream
        self._ck(B.lib().srt_occluded_rays_dev(self._h, C.c_void_p(r.data_ptr()), r.shape[0], C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def query_last(self):
        """the last ray-query launch (srt_query_last): dict(ms, waves, n_cached, narrow_refs, all_cached, paired, any); waits for that kernel"""
        q = B.QueryInfo()
        self._ck(B.lib().srt_query_last(self._h, C.byref(q)))
        return dict(ms=q.ms, waves=q.waves, n_cached=q.n_cached, narrow_refs=bool(q.narrow_refs), all_cached=bool(q.all_cached),
                    paired=bool(q.paired), any=bool(q.any))

    def set_query_test_grid(self, max_waves=0):
        """tests / tools only (srt_set_query_test_grid): at most max_waves persistent waves per query launch; 0 fills the device"""
        self._ck(B.lib().srt_set_query_test_grid(self._h, int(max_waves)))

    def direct_light(self, w, h, ox=0, oy=0, **cfg):
        """the deferred direct-light pass (srt_direct_light) over the w x h rectangle at (ox, oy) of the context's camera image, on the
        uploaded scene: dict(sum, m2, mean, stats) -- sum and m2 (h, w, 3) float32 XYZ sums over the call's samples of the contributions
        and of their squares, mean = sum / samples, stats = light_stats.  cfg: direct_light_config's arguments.  Reads only: no frame,
        accumulation or RNG state moves."""
        light = direct_light_config(**cfg)
        w, h, ox, oy = _motion_rect("Renderer.direct_light", w, h, ox, oy)
        s, m2, res = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32), B.LightResult()
        self._ck(B.lib().srt_direct_light(self._h, C.byref(light), B.fptr(s), B.fptr(m2), C.byref(res), w, h, ox, oy))
        return dict(sum=s, m2=m2, mean=s / np.float32(light.samples), stats=light_stats(res))

    def direct_light_kat(self, w, h, ox=0, oy=0, sample=0, **cfg):
        """one round of the sample index `sample` (srt_direct_light_kat): direct_light's dict and the round's device buffers copied out --
        cam_rows (n, 8), hit_rows (n, 4), light_rows (n, 8), sky_rows (n, 8) float32, records (n, 4) uint32 (bits of the weight, surface
        material, light index, kind | 4 light row traced | 8 sky row traced), occ_light, occ_sky (n,) bool; n = w h, row-major"""
        light = direct_light_config(samples=1, first_sample=sample, **cfg)
        w, h, ox, oy = _motion_rect("Renderer.direct_light_kat", w, h, ox, oy)
        n = w * h
        s, m2, res = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32), B.LightResult()
        cam, hits, lrows, srows = (np.zeros((n, k), np.float32) for k in (8, 4, 8, 8))
        rec, ol, os_ = np.zeros((n, 4), np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        u8 = C.POINTER(C.c_uint8)
        self._ck(B.lib().srt_direct_light_kat(self._h, C.byref(light), B.fptr(s), B.fptr(m2), C.byref(res), w, h, ox, oy, B.fptr(cam), B.fptr(hits),
                                              B.fptr(lrows), B.fptr(srows), rec.ctypes.data_as(C.POINTER(C.c_uint32)), ol.ctypes.data_as(u8),
                                              os_.ctypes.data_as(u8)))
        return dict(sum=s, m2=m2, mean=s.copy(), stats=light_stats(res), cam_rows=cam, hit_rows=hits, light_rows=lrows, sky_rows=srows,
                    records=rec, occ_light=ol.astype(bool), occ_sky=os_.astype(bool))

    def light_table(self):
        """the light table of the uploaded scene (srt_read_light_table): dict(thresholds (L + 1,) uint32, v0, e1, e2, normal (L, 3) float32,
        area (L,) float32, mat, tri, slot (L,) uint32)"""
        n = C.c_uint32(0)
        self._ck(B.lib().srt_read_light_table(self._h, C.byref(n), None, None, 0))
        L = n.value
        th, rec = np.zeros(L + 1, np.uint32), np.zeros((L, 16), np.float32)
        self._ck(B.lib().srt_read_light_table(self._h, C.byref(n), th.ctypes.data_as(C.POINTER(C.c_uint32)), B.fptr(rec), L))
        words = rec.view(np.uint32)
        return dict(thresholds=th, v0=rec[:, 0:3].copy(), area=rec[:, 3].copy(), e1=rec[:, 4:7].copy(), mat=words[:, 7].copy(),
                    e2=rec[:, 8:11].copy(), tri=words[:, 11].copy(), normal=rec[:, 12:15].copy(), slot=words[:, 15].copy())

    def direct_light_last(self):
        """kernel ms of the last direct-light call by kind (srt_direct_light_last): dict(camera_ms, shade_ms, gather_ms, query_ms, rounds,
        rows_per_round, query_launches)"""
        q = B.LightInfo()
        self._ck(B.lib().srt_direct_light_last(self._h, C.byref(q)))
        return dict(camera_ms=q.camera_ms, shade_ms=q.shade_ms, gather_ms=q.gather_ms, query_ms=q.query_ms, rounds=q.rounds,
                    rows_per_round=q.rows_per_round, query_launches=q.query_launches)

    def set_light_test_batch(self, max_rows=0):
        """tests / tools only (srt_set_light_test_batch): rounds of at most max_rows rows (one sample at least); 0 = the budget"""
        self._ck(B.lib().srt_set_light_test_batch(self._h, int(max_rows)))

    def op_sweep(self, which, a, b):
        a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
        out = np.zeros_like(a)
        self._ck(B.lib().srt_device_op_sweep(self._h, which, B.fptr(a), B.fptr(b), a.size, B.fptr(out)))
        return out

    def order_tiles_kat(self, cost, n_waves, split_load_pct=200, order_max_pct=0, guard=64):
        """the tile scheduler on explicit costs (srt_order_tiles_kat): cost = uint32[2 n], per-tile cost then the cost of each tile's most
        expensive pixel.  Returns (rows, sorted, info): the whole row buffer of 64 n + guard words, every word 0xffffffff before the
        kernel ran; the n tiles in queue order; [rows written, largest tile cost, 2 unused words]"""
        cost = np.ascontiguousarray(cost, np.uint32)
        n = cost.size // 2
        u32p = C.POINTER(C.c_uint32)
        rows, order, info = np.zeros(64 * n + guard, np.uint32), np.zeros(n, np.uint32), np.zeros(4, np.uint32)
        self._ck(B.lib().srt_order_tiles_kat(self._h, cost.ctypes.data_as(u32p), n, int(n_waves), int(split_load_pct), int(order_max_pct),
                                             rows.ctypes.data_as(u32p), rows.size, order.ctypes.data_as(u32p), info.ctypes.data_as(u32p)))
        return rows, order, info

    def tile_schedule(self, which=0):
        """the pixel queue of the last launch (srt_read_tile_schedule): which = 0 the cost probe's, which = 1 the compacted queue an
        adaptive pass left for the next one.  Returns (rows, info): uint32 queue rows and a dict of srt_tile_schedule_info's fields.
        SrtError when the last launch has no such queue.  Synchronises."""
        _, _, tl, _ = self.tile_buffer()
        rows, info = np.zeros(64 * tl, np.uint32), B.TileScheduleInfo()
        self._ck(B.lib().srt_read_tile_schedule(self._h, int(which), rows.ctypes.data_as(C.POINTER(C.c_uint32)), rows.size, C.byref(info)))
        return rows[:info.n_rows].copy(), {name: getattr(info, name) for name, _ in B.TileScheduleInfo._fields_ if name != "reserved"}


class Comm:
    """Multi-GPU communicator (srt_comm): W ranks render interleaved 8x8 tiles of a chunk, one RCCL gather to rank 0.
    Comm.init_all(devices): one process drives several GPUs.  Comm.init_rank(renderer, id, rank, world): one process per
    GPU, `id` from Comm.unique_id() on rank 0."""

    def __init__(self, handle, renderers, owns, ranks=None):
        self._h, self.renderers, self._owns = handle, renderers, owns
        self.ranks = list(range(len(renderers))) if ranks is None else list(ranks)      # the global rank of every local renderer
        self._offset = (0, 0)                                                            # image offset of the last frame's chunk
        self.world = B.lib().srt_comm_world(handle)

    @staticmethod
    def available():
        """True when an RCCL can be loaded in this process (no collective involved)"""
        return B.lib().srt_comm_available() == 0

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * B.COMM_ID_BYTES)()
        B.check_comm(B.lib().srt_comm_unique_id(buf))
        return bytes(buf)

    @classmethod
    def init_all(cls, devices):
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        B.check_comm(B.lib().srt_comm_init_all(arr, len(devices), C.byref(h)))
        rs = [Renderer(_borrowed=B.lib().srt_comm_ctx(h, k)) for k in range(B.lib().srt_comm_local_count(h))]
        return cls(h, rs, True)

    @classmethod
    def init_rank(cls, renderer, comm_id, rank, world):
        buf = (C.c_ubyte * B.COMM_ID_BYTES).from_buffer_copy(comm_id)
        h = C.c_void_p()
        B.check_comm(B.lib().srt_comm_init_rank(renderer._h, buf, rank, world, C.byref(h)))
        return cls(h, [renderer], False, [rank])

    def close(self):
        if getattr(self, "_h", None):
            B.lib().srt_comm_destroy(self._h)
            self._h = None
            for r in self.renderers:
                if not r._owned:
                    r._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, code):
        return B.check_comm(code, self._h)

    @property
    def root(self):
        """rank 0's renderer (holds the assembled framebuffer), None when rank 0 lives in another process"""
        p = B.lib().srt_comm_root_ctx(self._h)
        for r in self.renderers:
            if r._h and r._h.value == p:
                return r
        return None

    def upload_scene(self, scene):
        self._ck(B.lib().srt_comm_upload_scene(self._h, scene.handle))

    def set_camera(self, cam):
        self._ck(B.lib().srt_comm_set_camera(self._h, C.byref(cam)))

    def refit(self, vertices):
        """Renderer.refit with a numpy array on every local rank (srt_comm_refit_vertices), as upload_scene uploads to them"""
        v = refit_vertices("Comm.refit", vertices)
        self._ck(B.lib().srt_comm_refit_vertices(self._h, B.fptr(v), v.shape[0]))

    def init_device_params(self, chunk_w, chunk_h, spp, bounce_limit, seed=1984, tx=DEFAULT_TX, ty=DEFAULT_TY, bx=None, by=None):
        if bx is None or by is None:
            bx, by = reference_grid(chunk_w, chunk_h, tx, ty)
        self._ck(B.lib().srt_comm_init_device_params(self._h, tx, ty, bx, by, chunk_w, chunk_h, spp, bounce_limit, seed))
        for r in self.renderers:
            r.geom = dict(tx=tx, ty=ty, bx=bx, by=by, chunk_w=chunk_w, chunk_h=chunk_h, n_lanes=tx * ty * bx * by)

    def set_gather_planes(self, planes):
        self._ck(B.lib().srt_comm_set_gather_planes(self._h, planes))
        for r in self.renderers:
            r.gather_planes = planes

    def last_gather_ms(self):
        ms = C.c_float()
        self._ck(B.lib().srt_comm_last_gather_ms(self._h, C.byref(ms)))
        return ms.value

    def render_frame(self, width, height, offx=0, offy=0):
        self._ck(B.lib().srt_render_frame_multi(self._h, width, height, offx, offy))
        self._offset = (offx & 0xffff, offy & 0xffff)

    def accum_reset(self):
        """Renderer.accum_reset on every local rank"""
        self._ck(B.lib().srt_comm_accum_reset(self._h))

    def accum_reset_adaptive(self, rel_tol, abs_tol=0.0, min_spp=16):
        """Renderer.accum_reset_adaptive on every local rank (not on a process-per-GPU communicator: SrtError)"""
        self._ck(B.lib().srt_comm_accum_reset_adaptive(self._h, C.byref(adaptive_config(rel_tol, abs_tol, min_spp))))

    @property
    def accum_active(self):
        """active pixels summed over the local ranks"""
        n = C.c_uint64()
        self._ck(B.lib().srt_comm_accum_active(self._h, C.byref(n)))
        return n.value

    def accum_reset_spectral(self):
        """Renderer.accum_reset_spectral on every local rank; the films stay with their ranks until gather_accum(("film", ...))"""
        self._ck(B.lib().srt_comm_accum_reset_spectral(self._h))

    def accum_reset_features(self):
        """Renderer.accum_reset_features on every local rank (any communicator: no decision crosses ranks); the rows stay with their
        ranks (Renderer.read_features per context: each pixel is owned by one rank and reads +0 on the others) until gather_accum
        brings them to the root"""
        self._ck(B.lib().srt_comm_accum_reset_features(self._h))

    def accum_reset_adaptive_features(self, rel_tol, abs_tol=0.0, min_spp=16):
        """Renderer.accum_reset_adaptive_features on every local rank (not on a process-per-GPU communicator: SrtError); the rows stay
        with their ranks until gather_accum, as for accum_reset_features"""
        self._ck(B.lib().srt_comm_accum_reset_adaptive_features(self._h, C.byref(adaptive_config(rel_tol, abs_tol, min_spp))))

    def accum_reset_spectral_features(self):
        """Renderer.accum_reset_spectral_features on every local rank; film and rows stay with their ranks until gather_accum
        (the film only when it is asked for), as for accum_reset_spectral and accum_reset_features"""
        self._ck(B.lib().srt_comm_accum_reset_spectral_features(self._h))

    def accum_reset_adaptive_spectral(self, rel_tol, abs_tol=0.0, min_spp=16):
        """Renderer.accum_reset_adaptive_spectral on every local rank (single-process communicators only); the films stay with their ranks
        until gather_accum(("film", ...))"""
        self._ck(B.lib().srt_comm_accum_reset_adaptive_spectral(self._h, C.byref(adaptive_config(rel_tol, abs_tol, min_spp))))

    def accum_reset_adaptive_spectral_features(self, rel_tol, abs_tol=0.0, min_spp=16):
        """Renderer.accum_reset_adaptive_spectral_features on every local rank (single-process communicators only); films and rows stay
        with their ranks until gather_accum"""
        self._ck(B.lib().srt_comm_accum_reset_adaptive_spectral_features(self._h, C.byref(adaptive_config(rel_tol, abs_tol, min_spp))))

    def accum_reset_streams(self, k):
        """Renderer.accum_reset_streams on every local rank (any communicator: no decision crosses ranks)"""
        self._ck(B.lib().srt_comm_accum_reset_streams(self._h, int(k)))

    def _own_pixels(self, k, image_width, image_height):
        """(image_height, image_width) bool: the pixels of the last frame's chunk that lie in the 8 x 8 tiles local renderer k owns --
        tile (j // 8) * tiles_x + i // 8 of chunk pixel (i, j), tiles numbered over the whole reference grid, belongs to rank tile % world"""
        g = self.renderers[k].geom
        tiles_x = (g["tx"] * g["bx"] + 7) // 8
        i = np.arange(image_width, dtype=np.int64)[None, :] - self._offset[0]
        j = np.arange(image_height, dtype=np.int64)[:, None] - self._offset[1]
        return (i >= 0) & (j >= 0) & (((j // 8) * tiles_x + i // 8) % self.world == self.ranks[k])

    def _sum_of_own_pixels(self, image_width, image_height, read):
        """The frame's film or developed film from per-rank read-backs.  Where the root is local and whole for the film (after gather_accum,
        until its next pass) it holds the frame: its read-back alone.  Otherwise every local rank contributes the pixels of its OWN tiles
        and nothing else: a pixel of another rank reads +0 on a context that never gathered, and a STALE copy on a root that gathered
        before its last pass -- neither may enter the sum."""
        root = self.root
        if root is not None and root.accum_whole("film"):
            return read(root)
        out = None
        for k, r in enumerate(self.renderers):
            part = read(r)
            part = np.where(self._own_pixels(k, image_width, image_height)[..., None], part, np.zeros((), part.dtype))
            out = part if out is None else out + part
        return out

    def read_spectral(self, image_width, image_height, first=0, count=None):
        """the film of the frame (Renderer.read_spectral): on a single-process communicator (init_all) the sum over the local ranks of the
        film of each rank's OWN pixels, which is exact -- every pixel is owned by one rank; after gather_accum(("film", ...)), until the
        next pass, the root's film alone, which then holds every pixel (a root that gathered the film before its last pass keeps stale
        copies of the other ranks' pixels: they never enter the sum).  On a process-per-GPU communicator (init_rank) THIS rank's own
        pixels, +0 elsewhere -- except on a root that is whole for the film, which returns the frame's."""
        count = FILM_SAMPLES - first if count is None else count
        return self._sum_of_own_pixels(image_width, image_height, lambda r: r.read_spectral(image_width, image_height, first, count))

    def develop_spectral(self, image_width, image_height, response, scale=1.0, filter=None):
        """the developed film of the frame (Renderer.develop_spectral), put together as read_spectral puts the film together: the sum of
        every local rank's own pixels, or the root's result alone while the root is whole for the film; on a process-per-GPU
        communicator (init_rank) THIS rank's own pixels, zeros elsewhere, unless it is such a root"""
        resp = sensor_response(response, filter)
        return self._sum_of_own_pixels(image_width, image_height, lambda r: r.develop_spectral(image_width, image_height, resp, scale))

    def meter(self, with_hist=False, **cfg):
        """the frame metered over all ranks (Renderer.meter): the local ranks' histograms and counters are summed -- integers, and each
        rank meters the pixels of its own tiles only, so the sum is the whole frame's histogram exactly -- and srt_meter_decide decides
        on the sum.  While the root is whole (after gather_accum, until its next pass) its meter counts every pixel of the frame: then the
        root's metering alone is returned, and nothing is added to it.  Single-process communicators (init_all) only: on a
        process-per-GPU communicator the sum would need a reduction across processes (SrtError, SRT_ERR_UNSUPPORTED)."""
        if not self._owns:
            raise B.SrtError(-5, "Comm.meter: a process-per-GPU communicator cannot sum the ranks' histograms; meter every rank and reduce them yourself")
        m = meter_config(**cfg)
        whole = self.world > 1 and self.root.accum_whole()
        hist = np.zeros(METER_BINS, np.uint64)
        dark = nonfinite = 0
        for r in ([self.root] if whole else self.renderers):
            part = r.meter(with_hist=True, **cfg)
            hist += part["hist"]
            dark += part["dark"]
            nonfinite += part["nonfinite"]
        return meter_decide(hist, m, dark, nonfinite, with_hist)

    def render_frame_accum(self, width, height, spp_add, offx=0, offy=0):
        """render_frame with an accumulating pass of spp_add samples on every rank (Renderer.render_chunk_accum)"""
        self._ck(B.lib().srt_render_frame_multi_accum(self._h, width, height, offx, offy, spp_add))
        self._offset = (offx & 0xffff, offy & 0xffff)      # (the library's 16-bit chunk arguments, Q17)

    def gather_accum(self, parts=None):
        """the ranks' accumulations gathered on rank 0 (srt_comm_gather_accum; parts: gather_parts' names, a mask or None): afterwards
        the root runs every stage as a single context would -- until the next pass.  Asynchronous.  Returns Comm.root (None where rank
        0 lives in another process)."""
        self._ck(B.lib().srt_comm_gather_accum(self._h, gather_parts(parts)))
        return self.root

    def last_accum_gather_ms(self):
        """(pack_ms, exchange_ms, unpack_ms) of the last gather_accum (srt_comm_last_accum_gather_ms)"""
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        self._ck(B.lib().srt_comm_last_accum_gather_ms(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def synchronize(self):
        self._ck(B.lib().srt_comm_synchronize(self._h))

    def stats(self):
        rays, paths, ms = C.c_uint64(), C.c_uint64(), C.c_float()
        self._ck(B.lib().srt_comm_stats(self._h, C.byref(rays), C.byref(paths), C.byref(ms)))
        return dict(rays=rays.value, paths=paths.value, max_kernel_ms=ms.value)


GATHER_PARTS = B.GATHER_PARTS      # name -> SRT_GATHER_* bit (srt_c_api.h, srt_pack_accum)


def gather_parts(parts=None):
    """The SRT_GATHER_* mask of `parts`: None or 0 (everything the accumulation's kind holds except the film), a mask of the known bits,
    one name or an iterable of names out of GATHER_PARTS ("sums", "counts", "features", "film").  Anything else is refused here, before
    a device is touched."""
    known = sum(B.GATHER_PARTS.values())
    if parts is None:
        return 0
    if isinstance(parts, (bool, np.bool_)):
        raise TypeError("gather_parts: parts must be names, a mask or None, got %r" % (parts,))
    if isinstance(parts, (int, np.integer)):
        parts = int(parts)
        if parts < 0 or parts & ~known:
            raise ValueError("gather_parts: unknown bit(s) in mask %d (the parts are %s)" % (parts, ", ".join("%s = %d" % kv for kv in B.GATHER_PARTS.items())))
        return int(parts)
    names = [parts] if isinstance(parts, str) else list(parts)
    mask = 0
    for name in names:
        if not isinstance(name, str) or name not in B.GATHER_PARTS:
            raise ValueError("gather_parts: unknown part %r (the parts are %s)" % (name, ", ".join(B.GATHER_PARTS)))
        mask |= B.GATHER_PARTS[name]
    return mask


def pixels_per_lane(renderer, width, height, world=1):
    """pixels of a width x height frame per persistent lane of one rank's launch (CUs x waves per CU x 64 lanes; scene uploaded):
    below about 6 a launch is bound by its longest pixel chain, above by total work"""
    out = C.c_double()
    renderer._ck(B.lib().srt_pixels_per_lane(renderer._h, width, height, max(world, 1), C.byref(out)))
    return out.value


def tree_tuning(renderer, scene, width, height, bounce_limit, world=1, gate=False, segments=None):
    """srt_tune_tree_for_throughput (srt_c_api.h holds the recipe) as a dict of srt_tree_tuning's fields; gate: leave the tree of a
    launch with fewer than 6 pixels per lane untouched; segments: the caller's (n, 7) sample in place of the recorded one
    (srt_tune_tree_with_segments).  The scene is left uploaded; init_device_params comes next."""
    t = B.TreeTuning()
    if segments is None:
        renderer._ck(B.lib().srt_tune_tree_for_throughput(renderer._h, scene.handle, width, height, max(world, 1), bounce_limit, 1 if gate else 0, C.byref(t)))
    else:
        seg = ray_segments("tree_tuning", segments)
        renderer._ck(B.lib().srt_tune_tree_with_segments(renderer._h, scene.handle, width, height, max(world, 1), bounce_limit, 1 if gate else 0,
                                                         B.fptr(seg), seg.shape[0], C.byref(t)))
    return {name: getattr(t, name) for name, _ in B.TreeTuning._fields_}


def tune_tree_for_throughput(renderer, scene, width, height, bounce_limit, world=1, gate=False, segments=None):
    """Tree preparation for a THROUGHPUT-bound launch of a width x height frame on this build's own SAH tree (tree_tuning): insertion-based
    topology optimisation and the child order from a probe frame.  Not for launches with few pixels per lane (see pixels_per_lane): less
    total work is not a cheaper longest pixel -- measured 5-10 % slower there; gate=True leaves their tree as built.
    Returns a description for the record.  Deterministic: every rank arrives at the same tree."""
    t = tree_tuning(renderer, scene, width, height, bounce_limit, world, gate, segments)
    if gate and not t["throughput_bound"]:
        return "tree as built (chain-bound launch: fewer than 6 pixels per lane)"
    renderer._ck(t["order_status"])
    notes = {1: ["3 reinsertion passes"], 2: ["reinsertion undone (the deeper tree would no longer be LDS resident)"],
             3: ["3 reinsertion passes"],
             4: ["ray-weighted reinsertion vetoed (the sampled frame's work counters did not fall): tree as it walked in"],
             5: ["no usable ray segment in the sample: topology as it walked in"]}.get(t["reinsertion"], [])
    probe = (t["probe_width"], t["probe_height"], t["probe_spp"])
    notes.append(("child order profiled on a %dx%d x %d spp probe frame: %d nodes swapped" % (probe + (t["nodes_swapped"],))) if t["nodes_swapped"] else
                 ("builder's child order kept (the %dx%d x %d spp probe frame was not cheaper with the profiled one)" % probe))
    if t["reinsertion"] == 3:
        notes.append("reinsertion priced by %d sampled ray segments" % t["segments"])
    return "; ".join(notes)


# the recipe's probe frame for profile_child_order alone (tree_tuning takes it from the library): a quarter of the frame's size, at least
# 32 x 32, 8 spp, nodes with at least 16 deciding rays
PROFILE_PROBE = (4, 32, 8, 16)


def profile_child_order(renderer, scene, width, height, bounce_limit):
    """The tuning recipe's child-order step alone for a frame of width x height (tree_tuning, minus the reinsertion passes): the probe
    frame of the scene's default camera that srt_tune_tree_for_throughput uses.  Returns the number of nodes whose children were swapped
    (0: the probe frame was not cheaper with the profiled order and the builder's order was kept) and (probe width, height, spp)."""
    divisor, min_side, spp, min_samples = PROFILE_PROBE
    pw, ph = max(width // divisor, min_side), max(height // divisor, min_side)
    renderer.set_camera(scene.default_camera(pw, ph))
    return renderer.order_children_by_profile(scene, pw, ph, spp, bounce_limit, min_samples), (pw, ph, spp)


def render_image(scene, cam, width, height, spp, bounce_limit, seed=1984, device=0, count_traversal=False, renderer=None):
    """Whole-image single-chunk render on one GPU (the reference's default configuration, Q13).
    Returns dict with block-linear planes, row-major quantised planes, stats and kernel ms."""
    with _image_session(scene, cam, width, height, spp, bounce_limit, seed, device, renderer, count_traversal) as r:
        r.render_chunk(width, height, 0, 0)
        r.scatter_tiles()
        return _collect(r, width, height)


@contextlib.contextmanager
def _image_session(scene, cam, width, height, spp, bounce_limit, seed, device, renderer, count_traversal=False):
    """The set-up and tear-down every whole-image render on one GPU shares: `renderer` (or a new one on `device`, closed on exit) with
    scene, camera and device parameters in place, the whole frame as its partition and all nine planes as its exchange unit (restored
    on exit).  The planes are set before the caller's reset: a change of the planes ends an adaptive accumulation."""
    r = renderer or Renderer(device)
    planes_before = r.gather_planes
    try:
        r.upload_scene(scene)
        r.set_camera(cam)
        r.init_device_params(width, height, spp, bounce_limit, seed)
        r.set_partition(0, 1)
        r.set_count_traversal(count_traversal)
        r.set_gather_planes(9)            # the parity planes (unquantised sRGB, XYZ sums) are part of what the callers return
        yield r
    finally:
        if r._h:
            r.set_gather_planes(planes_before)
        if renderer is None:
            r.close()


def _collect(r, width, height):
    """the result dict of render_image from the frame `r` has just scattered"""
    return dict(fb=r.read_fb(), lin=r.read_fb_aux(1), xyz=r.read_fb_aux(2), rowmajor=r.read_fb_rowmajor(width, height),
                stats=r.stats(), kernel_ms=r.last_kernel_ms(), geom=dict(r.geom))


MAX_SPP = 65535      # the reference's spp is a short_uint (Q17): a progressive total cannot pass it either


def progressive_schedule(passes):
    """the samples of every pass as a list of ints, checked: at least one pass, every pass > 0, total <= MAX_SPP"""
    sched = [int(s) for s in passes]
    if not sched:
        raise ValueError("render_progressive: empty schedule (give the samples of at least one pass)")
    if any(s <= 0 for s in sched) or any(s != p for s, p in zip(sched, passes)):
        raise ValueError("render_progressive: every pass must add a positive whole number of samples, got %r" % (list(passes),))
    if sum(sched) > MAX_SPP:
        raise ValueError("render_progressive: %d samples in all, more than %d (16-bit spp)" % (sum(sched), MAX_SPP))
    return sched


def render_progressive(scene, cam, width, height, passes, bounce_limit, seed=1984, device=0, renderer=None):
    """Progressive whole-image render on one GPU: a generator that renders passes[0], passes[1], ... samples per pixel into one
    accumulation and yields (spp_total, result) after each pass, `result` with the keys of render_image.  After the pass that
    brings the total to N the result is bit-identical to render_image(..., spp=N, ...) (srt_render_chunk_accum).  The schedule is
    checked here, when the generator is made, before any device is touched."""
    sched = progressive_schedule(passes)
    return _progressive_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer)


def _progressive_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer):
    with _image_session(scene, cam, width, height, sum(sched), bounce_limit, seed, device, renderer) as r:
        r.accum_reset()
        for spp_add in sched:
            r.render_chunk_accum(width, height, spp_add)
            r.scatter_tiles()
            yield r.accum_samples, _collect(r, width, height)


MAX_STREAMS = 16      # SRT_MAX_STREAMS (srt_c_api.h)


def streams_schedule(passes, streams):
    """progressive_schedule for a streamed accumulation of `streams` streams per pixel, checked as the library checks it (ValueError):
    streams a whole number in [1, MAX_STREAMS] that divides every pass"""
    if isinstance(streams, bool) or not isinstance(streams, (int, np.integer)) or not 1 <= streams <= MAX_STREAMS:
        raise ValueError("render_streams: streams must be a whole number in [1, %d], got %r" % (MAX_STREAMS, streams))
    sched = progressive_schedule(passes)
    if any(s % streams for s in sched):
        raise ValueError("render_streams: every pass must be a multiple of the %d streams (each draws pass / streams samples), got %r" % (streams, sched))
    return sched


def render_streams(scene, cam, width, height, passes, bounce_limit, streams, seed=1984, device=0, renderer=None):
    """Progressive whole-image render with sample-parallel pixels on one GPU: a generator that renders passes[0], passes[1], ... samples
    per pixel, split evenly over `streams` independent RNG streams per pixel, into one accumulation and yields (spp_total, result)
    after each pass, as render_progressive does.  After the pass that brings the total to N, with n_lanes the lanes of the grid
    (result["geom"]), the XYZ sums are ((S_0 + S_1) + S_2) + ... in float32, S_k the XYZ sums of
    render_image(..., spp=N // streams, seed=seed + k * n_lanes), and the sRGB planes their plain conversion (srt_accum_reset_streams);
    streams=1 is render_progressive bit for bit.  The schedule is checked here, when the generator is made, before any device is
    touched."""
    sched = streams_schedule(passes, streams)
    return _streams_passes(scene, cam, width, height, sched, bounce_limit, int(streams), seed, device, renderer)


def _streams_passes(scene, cam, width, height, sched, bounce_limit, streams, seed, device, renderer):
    with _image_session(scene, cam, width, height, sum(sched), bounce_limit, seed, device, renderer) as r:
        r.accum_reset_streams(streams)
        for spp_add in sched:
            r.render_chunk_accum(width, height, spp_add)
            r.scatter_tiles()
            yield r.accum_samples, _collect(r, width, height)


def adaptive_config(rel_tol, abs_tol=0.0, min_spp=16):
    """srt_adaptive from Python numbers, checked as the library checks it (ValueError): min_spp a whole number >= 2, both tolerances
    finite and >= 0 in float32, and not both 0"""
    import math
    try:
        with np.errstate(over="ignore"):          # (a value beyond float32 becomes inf, refused below)
            rel, ab = float(np.float32(rel_tol)), float(np.float32(abs_tol))
    except (TypeError, ValueError):
        raise ValueError("adaptive sampling: rel_tol and abs_tol must be numbers, got %r, %r" % (rel_tol, abs_tol))
    if not (math.isfinite(rel) and math.isfinite(ab)) or rel < 0.0 or ab < 0.0 or not (rel + ab > 0.0):
        raise ValueError("adaptive sampling: rel_tol and abs_tol must be finite and >= 0, and not both 0; got %r, %r" % (rel_tol, abs_tol))
    if isinstance(min_spp, bool) or int(min_spp) != min_spp or not 2 <= int(min_spp) <= MAX_SPP:
        raise ValueError("adaptive sampling: min_spp must be a whole number in [2, %d], got %r" % (MAX_SPP, min_spp))
    return B.Adaptive(rel, ab, int(min_spp), 0)


def adaptive_schedule(min_spp, step, max_spp):
    """the samples of every pass of render_adaptive: max(min_spp, step) first, then step, the last pass clipped so that the total reaches
    max_spp exactly (fewer passes run when every pixel stops earlier).  Checked (ValueError)."""
    for name, v in (("min_spp", min_spp), ("step", step), ("max_spp", max_spp)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("render_adaptive: %s must be a whole number, got %r" % (name, v))
    if step <= 0:
        raise ValueError("render_adaptive: step must be > 0, got %r" % (step,))
    if not 2 <= min_spp <= max_spp:
        raise ValueError("render_adaptive: need 2 <= min_spp <= max_spp, got min_spp %r, max_spp %r" % (min_spp, max_spp))
    if max_spp > MAX_SPP:
        raise ValueError("render_adaptive: max_spp %d is more than %d (16-bit spp)" % (max_spp, MAX_SPP))
    sched = [min(max(min_spp, step), max_spp)]
    while sum(sched) < max_spp:
        sched.append(min(step, max_spp - sum(sched)))
    return [int(s) for s in sched]


def render_adaptive(scene, cam, width, height, bounce_limit, rel_tol, abs_tol=0.0, min_spp=16, step=16, max_spp=1024, seed=1984, device=0,
                    renderer=None):
    """Adaptive whole-image render on one GPU: a generator of (spp_total, active_pixels, result) after each pass, `result` with the keys
    of render_image plus `samples` (row-major uint32 map of the samples each pixel holds).  The first pass adds max(min_spp, step)
    samples, every later one `step` (the last clipped to reach max_spp); a pixel stops once the variance of its mean luminance is at
    most (rel_tol * mean + abs_tol)^2 (srt_c_api.h).  Stops when no pixel is active or max_spp is reached.  A pixel holding n samples is
    bit-identical to render_image(..., spp=n, ...) there.  The arguments are checked here, before any device is touched."""
    cfg = adaptive_config(rel_tol, abs_tol, min_spp)
    sched = adaptive_schedule(min_spp, step, max_spp)
    return _adaptive_passes(scene, cam, width, height, bounce_limit, cfg, sched, seed, device, renderer)


def _adaptive_passes(scene, cam, width, height, bounce_limit, cfg, sched, seed, device, renderer):
    with _image_session(scene, cam, width, height, sum(sched), bounce_limit, seed, device, renderer) as r:
        r._ck(B.lib().srt_accum_reset_adaptive(r._h, C.byref(cfg)))      # (after the session has set the planes)
        for spp_add in sched:
            r.render_chunk_accum(width, height, spp_add)
            r.scatter_tiles()
            active = r.accum_active
            out = _collect(r, width, height)
            out["samples"] = r.accum_stats(width, height)["samples"]
            yield r.accum_samples, active, out
            if active == 0:
                break


def spectral_wavelengths():
    """the 95 wavelengths of the spectral film's grid, 360 .. 830 nm in steps of 5, as float32"""
    return (360.0 + 5.0 * np.arange(FILM_SAMPLES)).astype(np.float32)


def spectral_radiance(film, samples, first=0):
    """mean spectral radiance per pixel from raw film sums (srt_c_api.h): L_j = F_j * 470 / (35 n) for 0 < j < 94 and twice that at the
    grid's ends j = 0 and j = 94, whose hats are half as wide.  film: (..., count) raw sums of grid samples first .. first + count - 1;
    samples: the samples n each pixel holds, a scalar or an array broadcastable to film[..., 0].  float64; NaN where n == 0."""
    film = np.asarray(film)
    j = first + np.arange(film.shape[-1])
    if first < 0 or j[-1] >= FILM_SAMPLES:
        raise ValueError("spectral_radiance: grid samples %d .. %d are outside 0 .. %d" % (first, j[-1], FILM_SAMPLES - 1))
    edge = np.where((j == 0) | (j == FILM_SAMPLES - 1), 2.0, 1.0)
    n = np.asarray(samples, np.float64)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return film.astype(np.float64) * (470.0 / 35.0) * edge / n


def film_to_xyz(film):
    """XYZ sums from a full film (..., 95): d * sum_j F_j * (x_j, y_j, z_j) with d = 470/7 (the kernel's float32 value) and the colour-matching
    rows of srt_color_tables, in float64.  Equals the accumulation's XYZ sums up to the reassociation of the float32 sums.  The same
    contraction with another sensor's curves on the grid is how a non-CIE response is applied."""
    film = np.asarray(film)
    if film.shape[-1] != FILM_SAMPLES:
        raise ValueError("film_to_xyz: needs all %d grid samples, got %d" % (FILM_SAMPLES, film.shape[-1]))
    cmf = np.zeros(FILM_SAMPLES * 4, np.float32)
    m = np.zeros(9, np.float32)
    B.check(B.lib().srt_color_tables(B.fptr(cmf), B.fptr(m)))
    xyz = cmf.reshape(FILM_SAMPLES, 4)[:, :3].astype(np.float64)
    return (film.astype(np.float64) @ xyz) * float(np.float32(470.0) / np.float32(7.0))


MAX_DEVELOP_CHANNELS = 16                                   # SRT_MAX_DEVELOP_CHANNELS (srt_c_api.h)
CIE_SCALE = float(np.float32(470.0) / np.float32(7.0))      # the kernel's float32 470/7: film_to_xyz's d


def cie_response():
    """the colour-matching rows x, y, z of srt_color_tables as response curves, float32 (3, 95)"""
    cmf = np.zeros(FILM_SAMPLES * 4, np.float32)
    m = np.zeros(9, np.float32)
    B.check(B.lib().srt_color_tables(B.fptr(cmf), B.fptr(m)))
    return np.ascontiguousarray(cmf.reshape(FILM_SAMPLES, 4)[:, :3].T)


def sensor_response(curves, filter=None):
    """response curves for Renderer.develop_spectral as a contiguous float32 (K, 95) array, checked as the library checks them
    (ValueError, before any device is touched): shape (K, 95) or (95,), 1 <= K <= MAX_DEVELOP_CHANNELS, every entry finite in float32.
    filter: 95 transmittances of a colour filter in front of the lens, finite, folded into every curve -- one float32 product per
    entry, R'[k][j] = R[k][j] * T_j."""
    try:
        with np.errstate(over="ignore"):
            r = np.array(curves, dtype=np.float32, ndmin=2)
    except (TypeError, ValueError):
        raise ValueError("sensor_response: the curves must be numbers in a (K, %d) or (%d,) array" % (FILM_SAMPLES, FILM_SAMPLES))
    if r.ndim != 2 or r.shape[1] != FILM_SAMPLES or not 1 <= r.shape[0] <= MAX_DEVELOP_CHANNELS:
        raise ValueError("sensor_response: needs (K, %d) or (%d,) curves with 1 <= K <= %d, got shape %r" % (FILM_SAMPLES, FILM_SAMPLES, MAX_DEVELOP_CHANNELS, np.shape(curves)))
    if not np.isfinite(r).all():
        raise ValueError("sensor_response: every response must be finite in float32")
    if filter is not None:
        try:
            with np.errstate(over="ignore"):
                t = np.array(filter, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError("sensor_response: the filter must be %d numbers" % FILM_SAMPLES)
        if t.shape != (FILM_SAMPLES,) or not np.isfinite(t).all():
            raise ValueError("sensor_response: the filter must be %d finite transmittances, got shape %r" % (FILM_SAMPLES, t.shape))
        with np.errstate(over="ignore"):
            r = (r * t).astype(np.float32)
        if not np.isfinite(r).all():
            raise ValueError("sensor_response: a filtered response overflows float32")
    return np.ascontiguousarray(r)


def _develop_scale(scale):
    """scale as a finite float32 held in a Python float (ValueError otherwise)"""
    try:
        if isinstance(scale, bool):
            raise TypeError
        with np.errstate(over="ignore"):
            s = float(np.float32(scale))
    except (TypeError, ValueError):
        raise ValueError("develop: scale must be a number, got %r" % (scale,))
    if not np.isfinite(s):
        raise ValueError("develop: scale must be finite in float32, got %r" % (scale,))
    return s


def render_developed(scene, cam, width, height, passes, bounce_limit, response=None, filter=None, scale=None, seed=1984, device=0, renderer=None):
    """render_spectral's passes with the film developed on the device behind every pass, without reading the film back: a generator of
    (spp_total, result, developed), `result` with the keys of render_image.  response=None: `developed` is the dict of
    Renderer.develop_spectral_srgb (the colour-matching rows, scale=None the float32 470/7) -- the picture through `filter`; else the
    (H, W, K) array of Renderer.develop_spectral(response, scale (None: 1), filter).  The develop only reads the accumulation, so result
    is render_spectral's bit for bit.  Schedule, curves, filter and scale are checked here, before any device is touched."""
    sched = progressive_schedule(passes)
    if response is None:
        resp = None if filter is None else sensor_response(cie_response(), filter)
    else:
        resp = sensor_response(response, filter)
    s = None if scale is None else _develop_scale(scale)
    return _developed_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, resp, response is None, s)


def _developed_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, resp, srgb, scale):
    with _image_session(scene, cam, width, height, sum(sched), bounce_limit, seed, device, renderer) as r:
        r.accum_reset_spectral()
        for spp_add in sched:
            r.render_chunk_accum(width, height, spp_add)
            r.scatter_tiles()
            out = _collect(r, width, height)
            if srgb:
                dev = r.develop_spectral_srgb(width, height, resp, scale)
            else:
                dev = r.develop_spectral(width, height, resp, 1.0 if scale is None else scale)
            yield r.accum_samples, out, dev


def render_spectral(scene, cam, width, height, passes, bounce_limit, seed=1984, device=0, renderer=None, first=0, count=FILM_SAMPLES):
    """Progressive whole-image render with a spectral film on one GPU: a generator of (spp_total, result, radiance) after each pass,
    `result` with the keys of render_image plus `film` (raw sums of grid samples [first, first + count), float32 (H, W, count)) and
    `radiance` = spectral_radiance(film, spp_total, first).  The colour planes after the pass that brings the total to N are
    bit-identical to render_image(..., spp=N, ...), as for render_progressive.  Checked before any device is touched."""
    sched = progressive_schedule(passes)
    if not (isinstance(first, (int, np.integer)) and isinstance(count, (int, np.integer))) or count <= 0 or first < 0 or first + count > FILM_SAMPLES:
        raise ValueError("render_spectral: [first, first + count) must be a non-empty part of 0 .. %d, got %r, %r" % (FILM_SAMPLES, first, count))
    return _spectral_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, int(first), int(count))


def _spectral_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, first, count):
    with _image_session(scene, cam, width, height, sum(sched), bounce_limit, seed, device, renderer) as r:
        r.accum_reset_spectral()
        for spp_add in sched:
            r.render_chunk_accum(width, height, spp_add)
            r.scatter_tiles()
            out = _collect(r, width, height)
            out["film"] = r.read_spectral(width, height, first, count)
            yield r.accum_samples, out, spectral_radiance(out["film"], r.accum_samples, first)


def split_features(rows):
    """(..., 8) first-hit rows -> dict(normal (..., 3), albedo (..., 3), distance (...), hits (...)), contiguous copies"""
    rows = np.asarray(rows)
    if rows.shape[-1] != FEATURE_CHANNELS:
        raise ValueError("split_features: needs rows of %d channels, got %d" % (FEATURE_CHANNELS, rows.shape[-1]))
    return dict(normal=np.ascontiguousarray(rows[..., 0:3]), albedo=np.ascontiguousarray(rows[..., 3:6]),
                distance=np.ascontiguousarray(rows[..., 6]), hits=np.ascontiguousarray(rows[..., 7]))


def feature_means(features, samples):
    """per-pixel means from the raw first-hit sums of read_features (srt_c_api.h), float64: normal and albedo divided by the samples n the
    pixel holds (a miss counts as a zero vector, so both fade with the coverage), distance divided by the hits (inf where no sample
    hit), and coverage = hits / n.  samples: a scalar or an array broadcastable to features["hits"]; NaN where n == 0."""
    n = np.asarray(samples, np.float64)
    hits = np.asarray(features["hits"], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(normal=np.asarray(features["normal"], np.float64) / n[..., None], albedo=np.asarray(features["albedo"], np.float64) / n[..., None],
                    distance=np.where(hits == 0, np.inf, np.asarray(features["distance"], np.float64) / hits), coverage=hits / n)


def render_features(scene, cam, width, height, passes, bounce_limit, seed=1984, device=0, renderer=None):
    """Progressive whole-image render with first-hit feature buffers on one GPU: a generator of (spp_total, result, features) after
    each pass, `result` with the keys of render_image and `features` the raw sums of read_features (feature_means(features, spp_total)
    normalises them).  The colour planes after the pass that brings the total to N are bit-identical to render_image(..., spp=N, ...),
    as for render_progressive.  Checked before any device is touched."""
    sched = progressive_schedule(passes)
    return _features_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer)


def _features_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer):
    with _image_session(scene, cam, width, height, sum(sched), bounce_limit, seed, device, renderer) as r:
        r.accum_reset_features()
        for spp_add in sched:
            r.render_chunk_accum(width, height, spp_add)
            r.scatter_tiles()
            yield r.accum_samples, _collect(r, width, height), r.read_features(width, height)


METER_BINS = 4096      # SRT_METER_BINS (srt_c_api.h)
_METER_KEYS = ("rect", "percentile_ppm", "key", "gain_min", "gain_max")
_TONE_KEYS = ("curve", "white")
CURVES = {"linear": 0, "reinhard": 1}


def _expose_number(who, name, v):
    """v as a float32 held in a Python float (a value beyond float32 becomes inf); ValueError for what is no number"""
    try:
        if isinstance(v, bool):
            raise TypeError
        with np.errstate(over="ignore"):
            return float(np.float32(v))
    except (TypeError, ValueError):
        raise ValueError("%s: %s must be a number, got %r" % (who, name, v))


def meter_config(rect=None, percentile_ppm=500000, key=0.18, gain_min=2.0 ** -24, gain_max=2.0 ** 24):
    """srt_meter from Python numbers, checked as the library checks it (ValueError): rect None -- the whole chunk -- or (x0, y0, w, h) in
    chunk pixels, non-empty (the library checks it against the chunk); percentile_ppm a whole number in [1, 1000000], the percentile of
    the metered luminances, in parts per million, whose bin is anchored at key; key finite and > 0; 0 < gain_min <= gain_max, finite.
    The defaults -- the median anchored at 0.18, gains within 2^-24 .. 2^24 -- are starting values, untuned."""
    if isinstance(percentile_ppm, bool) or not isinstance(percentile_ppm, (int, np.integer)) or not 1 <= percentile_ppm <= 1000000:
        raise ValueError("meter: percentile_ppm must be a whole number in [1, 1000000], got %r" % (percentile_ppm,))
    k, lo, hi = (_expose_number("meter", n, v) for n, v in (("key", key), ("gain_min", gain_min), ("gain_max", gain_max)))
    if not (np.isfinite(k) and k > 0.0):
        raise ValueError("meter: key must be finite and > 0 in float32, got %r" % (key,))
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= hi):
        raise ValueError("meter: needs 0 < gain_min <= gain_max, both finite in float32, got %r, %r" % (gain_min, gain_max))
    if rect is None:
        rect = (0, 0, 0, 0)
    else:
        rect = tuple(rect)
        if len(rect) != 4 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < 2 ** 32 for v in rect) or rect[2] == 0 or rect[3] == 0:
            raise ValueError("meter: rect must be None or (x0, y0, w, h) of whole numbers with w > 0 and h > 0, got %r" % (rect,))
    return B.Meter(int(rect[0]), int(rect[1]), int(rect[2]), int(rect[3]), int(percentile_ppm), k, lo, hi, (C.c_uint32 * 4)(0, 0, 0, 0))


def tone_config(gain=1.0, curve="reinhard", white=4.0):
    """srt_tone from Python numbers, checked as the library checks it (ValueError): gain finite and > 0 in float32 (what meter() decided,
    or the caller's own); curve "linear" (0) or "reinhard" (1: extended Reinhard on luminance); white > 0, the luminance after the gain
    that the curve maps to 1 (inf: plain Reinhard).  curve and white = 4 are starting values, untuned."""
    if isinstance(curve, str):
        if curve not in CURVES:
            raise ValueError("tone: curve must be one of %s (or 0, 1), got %r" % (sorted(CURVES), curve))
        curve = CURVES[curve]
    if isinstance(curve, bool) or not isinstance(curve, (int, np.integer)) or curve not in (0, 1):
        raise ValueError("tone: curve must be 0 (linear) or 1 (reinhard), got %r" % (curve,))
    g, w = _expose_number("tone", "gain", gain), _expose_number("tone", "white", white)
    if not (np.isfinite(g) and g > 0.0):
        raise ValueError("tone: gain must be finite and > 0 in float32, got %r" % (gain,))
    if not w > 0.0:
        raise ValueError("tone: white must be > 0 in float32 (inf allowed), got %r" % (white,))
    return B.Tone(int(curve), g, w, (C.c_uint32 * 5)(0, 0, 0, 0, 0))


def _split_expose_cfg(cfg):
    """(meter keywords, tone keywords) of expose()'s cfg; TypeError for a name that is neither"""
    unknown = sorted(set(cfg) - set(_METER_KEYS) - set(_TONE_KEYS))
    if unknown:
        raise TypeError("expose: unknown keyword(s) %s (meter: %s; tone: %s)" % (", ".join(unknown), ", ".join(_METER_KEYS), ", ".join(_TONE_KEYS)))
    return {k: v for k, v in cfg.items() if k in _METER_KEYS}, {k: v for k, v in cfg.items() if k in _TONE_KEYS}


def _xyz_image(who, xyz_mean):
    img = np.ascontiguousarray(xyz_mean, np.float32)
    if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] == 0 or img.shape[1] == 0:
        raise ValueError("%s: needs an XYZ-mean image (h, w, 3) with h, w >= 1, got %r" % (who, img.shape))
    return img


def _meter_dict(res, hist=None):
    out = dict(metered=res.metered, dark=res.dark, nonfinite=res.nonfinite, bin_ref=res.bin_ref, y_ref=res.y_ref, gain=res.gain)
    if hist is not None:
        out["hist"] = hist
    return out


def meter_decide(hist, cfg=None, dark=0, nonfinite=0, with_hist=False):
    """the exposure decided from a luminance histogram on the host (srt_meter_decide; needs no GPU): hist 4096 counts, each below 2^32 --
    one context's, or the sum of the histograms of a partition's ranks; cfg a meter_config() (None: the defaults) -> the dict of
    Renderer.meter, dark and nonfinite passed through."""
    h = np.asarray(hist)
    if h.shape != (METER_BINS,) or h.dtype.kind not in "iu" or (h < 0).any() or (h >= 2 ** 32).any():
        raise ValueError("meter_decide: needs %d whole counts in [0, 2^32)" % METER_BINS)
    h32 = np.ascontiguousarray(h, np.uint32)
    res = B.MeterResult(0, int(dark), int(nonfinite), 0, 0.0, 0.0, 0)
    m = meter_config() if cfg is None else cfg
    B.check(B.lib().srt_meter_decide(h32.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(m), C.byref(res)))
    return _meter_dict(res, h32 if with_hist else None)


def render_exposed(scene, cam, width, height, passes, bounce_limit, gain=None, seed=1984, device=0, renderer=None, **cfg):
    """render_progressive with the exposure metered and the picture toned on the device behind every pass: a generator of (spp_total,
    result, meter, exposed) -- `result` with the keys of render_image, `exposed` the dict of Renderer.expose (cfg: the keywords of
    meter_config and tone_config) and `meter` its metering (None with an explicit gain).  Metering and toning only read the
    accumulation, so result is render_progressive's bit for bit.  Schedule and cfg are checked here, before any device is touched."""
    sched = progressive_schedule(passes)
    mcfg, tcfg = _split_expose_cfg(cfg)
    meter_config(**mcfg)
    tone_config(gain=1.0 if gain is None else gain, **tcfg)
    if gain is not None and mcfg:
        raise ValueError("render_exposed: %s given with an explicit gain, which is not metered" % ", ".join(sorted(mcfg)))
    return _exposed_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, gain, cfg)


def _exposed_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, gain, cfg):
    with _image_session(scene, cam, width, height, sum(sched), bounce_limit, seed, device, renderer) as r:
        r.accum_reset()
        for spp_add in sched:
            r.render_chunk_accum(width, height, spp_add)
            r.scatter_tiles()
            out = _collect(r, width, height)
            exposed = r.expose(width, height, gain, **cfg)
            yield r.accum_samples, out, exposed["meter"], exposed


_DESPECKLE_KEYS = ("radius", "rank_ppm", "gain", "floor")


def despeckle_config(radius=2, rank_ppm=875000, gain=4.0, floor=None):
    """srt_despeckle from Python numbers, checked as the library checks it (ValueError): radius 1 or 2, the window is (2 radius + 1)^2
    pixels without its centre; rank_ppm a whole number in [0, 1000000], the rank of the reference neighbour in parts per million of
    m - 1 (500000: the lower median; 875000: with 24 neighbours the 4th largest, which keeps a one-pixel-wide line; 1000000: the
    largest); gain finite and >= 0 in float32; floor >= 0 in float32 (inf switches the filter off) or None.  A pixel is clamped to
    limit = gain * reference + floor.  floor None stands for a metered floor: the struct holds 0, and the Renderer methods that take
    these keywords put the median luminance bin of the lit pixels there (meter(percentile_ppm=500000)["y_ref"]), without which a
    sparse picture -- most neighbours black -- is clamped to black.  The defaults are starting values, untuned."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or radius not in (1, 2):
        raise ValueError("despeckle: radius must be 1 or 2, got %r" % (radius,))
    if isinstance(rank_ppm, bool) or not isinstance(rank_ppm, (int, np.integer)) or not 0 <= rank_ppm <= 1000000:
        raise ValueError("despeckle: rank_ppm must be a whole number in [0, 1000000], got %r" % (rank_ppm,))
    g = _expose_number("despeckle", "gain", gain)
    if not (np.isfinite(g) and g >= 0.0):
        raise ValueError("despeckle: gain must be finite and >= 0 in float32, got %r" % (gain,))
    f = 0.0 if floor is None else _expose_number("despeckle", "floor", floor)
    if not f >= 0.0:
        raise ValueError("despeckle: floor must be >= 0 in float32 (inf switches the filter off) or None (metered), got %r" % (floor,))
    return B.Despeckle(int(radius), int(rank_ppm), g, f, (C.c_uint32 * 4)(0, 0, 0, 0))


def render_despeckled(scene, cam, width, height, passes, bounce_limit, denoise=True, despeckle=None, seed=1984, device=0, renderer=None, **cfg):
    """render_features with the firefly filter behind every pass: a generator of (spp_total, result, features, cleaned) -- with
    denoise=True `cleaned` is the dict of Renderer.denoise_despeckled (cfg: the keywords of denoise_config), else the dict of
    Renderer.despeckle (no cfg); despeckle: a dict of the keywords of despeckle_config, None: the defaults.  The filter only reads the
    accumulation, so result and features are render_features' bit for bit.  Schedule and configurations are checked here, before any
    device is touched."""
    sched = progressive_schedule(passes)
    kw = dict(despeckle or {})
    unknown = sorted(set(kw) - set(_DESPECKLE_KEYS))
    if unknown:
        raise TypeError("render_despeckled: unknown despeckle keyword(s) %s (%s)" % (", ".join(unknown), ", ".join(_DESPECKLE_KEYS)))
    despeckle_config(**kw)
    if denoise:
        denoise_config(**cfg)
    elif cfg:
        raise TypeError("render_despeckled: %s given with denoise=False, which runs no denoiser" % ", ".join(sorted(cfg)))
    return _despeckled_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, bool(denoise), kw, cfg)


def _despeckled_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, denoise, despeckle, cfg):
    with _image_session(scene, cam, width, height, sum(sched), bounce_limit, seed, device, renderer) as r:
        r.accum_reset_features()
        for spp_add in sched:
            r.render_chunk_accum(width, height, spp_add)
            r.scatter_tiles()
            cleaned = r.denoise_despeckled(width, height, despeckle, **cfg) if denoise else r.despeckle(width, height, **despeckle)
            yield r.accum_samples, _collect(r, width, height), r.read_features(width, height), cleaned


_TEMPORAL_KEYS = ("alpha_min", "max_len", "sigma_normal", "sigma_albedo", "sigma_depth")


def temporal_config(alpha_min=0.1, max_len=32, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1):
    """srt_temporal from Python numbers, checked as the library checks it (ValueError): alpha_min in (0, 1] in float32, the floor of the
    blend weight (1 switches the blend off); max_len finite and >= 1, the cap of the history length (the weight of a new frame is
    1 / len, so 32 frames of history weigh a new one at 1/32 before the floor); every sigma > 0 in float32 and not NaN (inf switches its
    test off): a history tap is rejected when its normal or albedo differs from the pixel's by more than the sigma (Euclidean), or its
    stored distance from the expected one by more than sigma_depth relative.  The defaults are starting values, untuned."""
    vals = []
    for name, v in zip(_TEMPORAL_KEYS, (alpha_min, max_len, sigma_normal, sigma_albedo, sigma_depth)):
        vals.append(_expose_number("temporal", name, v))
    a, m = vals[0], vals[1]
    if not (a > 0.0 and a <= 1.0):
        raise ValueError("temporal: alpha_min must be in (0, 1] in float32, got %r" % (alpha_min,))
    if not (m >= 1.0 and np.isfinite(m)):
        raise ValueError("temporal: max_len must be finite and >= 1 in float32, got %r" % (max_len,))
    for name, f, v in zip(_TEMPORAL_KEYS[2:], vals[2:], (sigma_normal, sigma_albedo, sigma_depth)):
        if not f > 0.0:
            raise ValueError("temporal: %s must be > 0 in float32 (inf switches the test off), got %r" % (name, v))
    return B.Temporal(a, m, vals[2], vals[3], vals[4], (C.c_uint32 * 3)(0, 0, 0))


def _temporal_cfg(who, temporal):
    """srt_temporal from a dict of the keywords of temporal_config (None: the defaults); TypeError for a name that is none of them"""
    kw = dict(temporal or {})
    unknown = sorted(set(kw) - set(_TEMPORAL_KEYS))
    if unknown:
        raise TypeError("%s: unknown temporal keyword(s) %s (%s)" % (who, ", ".join(unknown), ", ".join(_TEMPORAL_KEYS)))
    return temporal_config(**kw)


MAX_TEMPORAL_MIN_LEN = 2 ** 24


def temporal_vg_config(min_len=4, moving=False):
    """srt_temporal_vg from Python values, checked as the library checks it (ValueError): min_len a whole number in [2, 2^24] -- the
    moments' own history length from which a pixel's filter is guided by the variance measured across frames instead of the spatial
    estimate (above the stage's max_len: never); moving a bool -- the moving stage, which needs tracking on.  min_len = 4 is a starting
    value, untuned."""
    if isinstance(min_len, bool) or not isinstance(min_len, (int, np.integer)) or not 2 <= min_len <= MAX_TEMPORAL_MIN_LEN:
        raise ValueError("temporal_vg: min_len must be a whole number in [2, 2^24], got %r" % (min_len,))
    if not isinstance(moving, (bool, np.bool_)):
        raise ValueError("temporal_vg: moving must be a bool, got %r" % (moving,))
    return B.TemporalVG(int(min_len), 1 if moving else 0, (C.c_uint32 * 2)(0, 0))


def temporal_stats(res):
    """srt_temporal_result as a dict: the pixels blended, fresh (of those: offscreen, rejected) and nonfinite, history_frames (the calls
    since the history began, this one included) and history_dropped (this call discarded a history of another rectangle)"""
    return dict(blended=res.blended, fresh=res.fresh, offscreen=res.offscreen, rejected=res.rejected, nonfinite=res.nonfinite,
                history_frames=res.history_frames, history_dropped=bool(res.history_dropped))


def motion_stats(res):
    """srt_motion_result as a dict: the pixels whose centre ray hit and missed, the hit pixels whose triangle moved, and of those the
    degenerate ones (no previous point could be formed)"""
    return dict(hit=res.hit, miss=res.miss, moved=res.moved, degenerate=res.degenerate)


def light_stats(res):
    """srt_light_result as a dict: the samples that missed, saw an emitter, met a specular surface and were shaded, the traced light and
    sky rows and the unoccluded ones among them, and the lights in the table"""
    return {k: int(getattr(res, k)) for k in ("miss", "emitted", "specular", "shaded", "light_rows", "light_unoccluded", "sky_rows",
                                                "sky_unoccluded", "lights")}


def direct_light_config(samples=16, seed=0, first_sample=0, parts=("emitted", "lights", "sky")):
    """srt_light, checked as the library checks it (ValueError) before any library call: samples 1 .. 65536, first_sample + samples at
    most 2^32, seed below 2^64, parts a non-empty collection of "emitted", "lights", "sky" """
    for name, v, hi in (("samples", samples, B.LIGHT_MAX_SAMPLES), ("seed", seed, 2 ** 64 - 1), ("first_sample", first_sample, 2 ** 32 - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 or v > hi:
            raise ValueError("direct_light_config: %s must be an integer in 0 .. %d, got %r" % (name, hi, v))
    if samples < 1:
        raise ValueError("direct_light_config: samples must be at least 1")
    if first_sample + samples > 2 ** 32:
        raise ValueError("direct_light_config: first_sample + samples must not exceed 2^32")
    if isinstance(parts, str):
        parts = (parts,)
    parts = tuple(parts)
    if not parts or any(p not in B.LIGHT_PARTS for p in parts):
        raise ValueError("direct_light_config: parts must name at least one of %s, got %r" % (sorted(B.LIGHT_PARTS), parts))
    mask = 0
    for p in parts:
        mask |= B.LIGHT_PARTS[p]
    return B.Light(samples=int(samples), first_sample=int(first_sample), parts=mask, reserved=0, seed=int(seed))


def render_direct(scene, cam, width, height, passes, samples=16, device=0, renderer=None, **cfg):
    """Direct-lighting preview of the whole image on one GPU: a generator that runs `passes` calls of `samples` samples each, advancing
    first_sample, and yields (samples_total, mean, stats) after each -- mean (height, width, 3) float32 XYZ of all samples so far, stats
    the counters summed.  The mean goes through expose_kat / present_kat / despeckle_kat as any XYZ mean does.  The arguments are checked
    here, when the generator is made, before any device is touched."""
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or passes < 1:
        raise ValueError("render_direct: passes must be a positive integer, got %r" % (passes,))
    first = int(cfg.pop("first_sample", 0))
    for k in range(int(passes)):
        direct_light_config(samples=samples, first_sample=first + k * samples, **cfg)
    return _direct_passes(scene, cam, int(width), int(height), int(passes), int(samples), first, device, renderer, cfg)


def _direct_passes(scene, cam, width, height, passes, samples, first, device, renderer, cfg):
    r = renderer or Renderer(device)
    try:
        r.upload_scene(scene)
        r.set_camera(cam)
        total = np.zeros((height, width, 3), np.float64)
        stats = None
        for k in range(passes):
            out = r.direct_light(width, height, samples=samples, first_sample=first + k * samples, **cfg)
            total += out["sum"]
            stats = out["stats"] if stats is None else {n: (v if n == "lights" else v + stats[n]) for n, v in out["stats"].items()}
            done = (k + 1) * samples
            yield done, (total / done).astype(np.float32), stats
    finally:
        if renderer is None:
            r.close()


def _motion_rect(who, w, h, ox, oy):
    """the rectangle of a motion pass as the library checks it (ValueError), before any library call"""
    vals = []
    for name, v in (("w", w), ("h", h), ("ox", ox), ("oy", oy)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError("%s: %s must be a non-negative integer, got %r" % (who, name, v))
        vals.append(int(v))
    w, h, ox, oy = vals
    if w == 0 or h == 0 or w * h >= 2 ** 31:
        raise ValueError("%s: w x h must be in 1 .. 2^31 - 1, got %d x %d" % (who, w, h))
    if ox + w > 2 ** 24 or oy + h > 2 ** 24:
        raise ValueError("%s: ox + w and oy + h must not exceed 2^24, got %d and %d" % (who, ox + w, oy + h))
    return w, h, ox, oy


def _variance_guided_cfg(who, variance_guided, denoise, cfg):
    """render_interactive's / render_animated's variance_guided=True: cfg holds min_len and the keywords of denoise_vg_config; both are
    checked here.  (min_len, the rest of cfg)"""
    if not isinstance(variance_guided, (bool, np.bool_)):
        raise TypeError("%s: variance_guided must be a bool, got %r" % (who, variance_guided))
    if not variance_guided:
        return None, cfg
    if not denoise:
        raise ValueError("%s: variance_guided=True with denoise=False: the variance guides the denoiser" % who)
    rest = dict(cfg)
    min_len = rest.pop("min_len", 4)
    temporal_vg_config(min_len)
    denoise_vg_config(**rest)
    return min_len, rest


def render_interactive(scene, cameras, width, height, spp, bounce_limit, denoise=True, despeckle=None, temporal=None, seed=1984, device=0, renderer=None,
                       variance_guided=False, **cfg):
    """A moving camera on one GPU: for every camera of `cameras` (CameraData, at least one) set_camera, accum_reset_features, one pass of
    `spp` samples, then the chained call that carries the picture over from the previous camera -- denoise=True:
    Renderer.denoise_temporal(width, height, temporal, despeckle, **cfg) (cfg: the keywords of denoise_config), else
    Renderer.temporal(width, height, **temporal) (no cfg, no despeckle).  A generator of (index, result, features, picture, stats):
    `result` with the keys of render_image, `features` the raw sums of read_features, `picture` the chained call's dict, `stats` its
    temporal_stats.  The history starts with the first camera (temporal_reset).  Everything is checked here, before any device is
    touched.
    variance_guided=True (with denoise=True) uses Renderer.denoise_temporal_vg in the chained call's place: cfg then holds min_len and the
    keywords of denoise_vg_config, and `picture` gains var and n_temporal."""
    min_len, cfg = _variance_guided_cfg("render_interactive", variance_guided, denoise, cfg)
    cams = list(cameras)
    if not cams:
        raise ValueError("render_interactive: no camera (give at least one)")
    for k, cam in enumerate(cams):
        if not isinstance(cam, B.CameraData):
            raise TypeError("render_interactive: cameras[%d] is no CameraData (camera_init makes one), got %r" % (k, type(cam).__name__))
    sched = progressive_schedule([spp])
    tkw = dict(temporal or {})
    _temporal_cfg("render_interactive", tkw)
    dkw = None
    if despeckle is not None:
        dkw = dict(despeckle)
        unknown = sorted(set(dkw) - set(_DESPECKLE_KEYS))
        if unknown:
            raise TypeError("render_interactive: unknown despeckle keyword(s) %s (%s)" % (", ".join(unknown), ", ".join(_DESPECKLE_KEYS)))
        despeckle_config(**dkw)
    if min_len is not None:
        return _interactive_frames_vg(scene, cams, width, height, sched[0], bounce_limit, seed, device, renderer, dkw, tkw, min_len, cfg)
    if denoise:
        denoise_config(**cfg)
    elif cfg:
        raise TypeError("render_interactive: %s given with denoise=False, which runs no denoiser" % ", ".join(sorted(cfg)))
    elif dkw is not None:
        raise ValueError("render_interactive: despeckle given with denoise=False: the firefly filter runs in the denoiser's chain")
    return _interactive_frames(scene, cams, width, height, sched[0], bounce_limit, seed, device, renderer, bool(denoise), dkw, tkw, cfg)


def _interactive_frames(scene, cams, width, height, spp, bounce_limit, seed, device, renderer, denoise, despeckle, temporal, cfg):
    with _image_session(scene, cams[0], width, height, spp, bounce_limit, seed, device, renderer) as r:
        r.temporal_reset()
        for k, cam in enumerate(cams):
            r.set_camera(cam)
            r.accum_reset_features()
            r.render_chunk_accum(width, height, spp)
            r.scatter_tiles()
            picture = r.denoise_temporal(width, height, temporal, despeckle, **cfg) if denoise else r.temporal(width, height, **temporal)
            yield k, _collect(r, width, height), r.read_features(width, height), picture, picture["stats"]


def _interactive_frames_vg(scene, cams, width, height, spp, bounce_limit, seed, device, renderer, despeckle, temporal, min_len, cfg):
    with _image_session(scene, cams[0], width, height, spp, bounce_limit, seed, device, renderer) as r:
        r.temporal_reset()
        for k, cam in enumerate(cams):
            r.set_camera(cam)
            r.accum_reset_features()
            r.render_chunk_accum(width, height, spp)
            r.scatter_tiles()
            picture = r.denoise_temporal_vg(width, height, temporal, despeckle, min_len, False, **cfg)
            yield k, _collect(r, width, height), r.read_features(width, height), picture, picture["stats"]


def render_interactive_multi(scene, cameras, width, height, spp, bounce_limit, devices=None, comm=None, denoise=True, despeckle=None, temporal=None,
                             variance_guided=False, seed=1984, **cfg):
    """render_interactive on several GPUs: for every camera Comm.set_camera, accum_reset_features, one render_frame_accum of `spp`
    samples on every rank's own tiles, Comm.gather_accum, then render_interactive's chained call on the root, which holds the whole
    accumulation.  `comm` (a single-process communicator, left open) or `devices` (Comm.init_all, closed at the end; None: device 0
    alone).  Yields what render_interactive yields -- the same bits, whatever the number of ranks; `stats` of `result` are the root's
    own with rays and paths summed over the ranks.  Everything is checked here, before any device is touched."""
    who = "render_interactive_multi"
    min_len, cfg = _variance_guided_cfg(who, variance_guided, denoise, cfg)
    cams = list(cameras)
    if not cams:
        raise ValueError("%s: no camera (give at least one)" % who)
    for k, cam in enumerate(cams):
        if not isinstance(cam, B.CameraData):
            raise TypeError("%s: cameras[%d] is no CameraData (camera_init makes one), got %r" % (who, k, type(cam).__name__))
    if comm is not None and devices is not None:
        raise ValueError("%s: give comm or devices, not both" % who)
    if comm is not None and (not isinstance(comm, Comm) or not comm._owns):
        raise TypeError("%s: comm must be a single-process Comm (Comm.init_all): the root runs the chain and collects the frame" % who)
    spp = progressive_schedule([spp])[0]
    tkw = dict(temporal or {})
    _temporal_cfg(who, tkw)
    dkw = None
    if despeckle is not None:
        dkw = dict(despeckle)
        unknown = sorted(set(dkw) - set(_DESPECKLE_KEYS))
        if unknown:
            raise TypeError("%s: unknown despeckle keyword(s) %s (%s)" % (who, ", ".join(unknown), ", ".join(_DESPECKLE_KEYS)))
        despeckle_config(**dkw)
    if min_len is None:
        if denoise:
            denoise_config(**cfg)
        elif cfg:
            raise TypeError("%s: %s given with denoise=False, which runs no denoiser" % (who, ", ".join(sorted(cfg))))
        elif dkw is not None:
            raise ValueError("%s: despeckle given with denoise=False: the firefly filter runs in the denoiser's chain" % who)
    return _interactive_frames_multi(scene, cams, width, height, spp, bounce_limit, seed, devices, comm, bool(denoise), dkw, tkw, min_len, cfg)


def _interactive_frames_multi(scene, cams, width, height, spp, bounce_limit, seed, devices, comm, denoise, despeckle, temporal, min_len, cfg):
    c = comm or Comm.init_all(list(devices) if devices is not None else [0])
    planes_before = c.renderers[0].gather_planes
    try:
        c.upload_scene(scene)
        c.set_camera(cams[0])
        c.init_device_params(width, height, spp, bounce_limit, seed)
        c.set_gather_planes(9)            # the parity planes are part of what the frames return (as _image_session)
        root = c.root
        root.temporal_reset()
        for k, cam in enumerate(cams):
            c.set_camera(cam)
            c.accum_reset_features()
            c.render_frame_accum(width, height, spp)
            c.gather_accum()
            if min_len is not None:
                picture = root.denoise_temporal_vg(width, height, temporal, despeckle, min_len, False, **cfg)
            else:
                picture = root.denoise_temporal(width, height, temporal, despeckle, **cfg) if denoise else root.temporal(width, height, **temporal)
            result = _collect(root, width, height)
            total = c.stats()
            result["stats"]["rays"], result["stats"]["paths"] = total["rays"], total["paths"]
            yield k, result, root.read_features(width, height), picture, picture["stats"]
    finally:
        if comm is None:
            c.close()
        elif c._h:
            c.set_gather_planes(planes_before)


def render_animated(scene, cam, frames, width, height, spp, bounce_limit, denoise=True, despeckle=None, temporal=None, seed=1984, device=0,
                    renderer=None, track_motion=False, variance_guided=False, **cfg):
    """Moving geometry on one GPU: the scene is uploaded once; for every vertex array of `frames` ((n_tris, 3, 3) float32: numpy, or a
    torch tensor on the device -- Renderer.refit) refit, accum_reset_features, one pass of `spp` samples, then the chained presentation
    call of render_interactive (denoise, despeckle, temporal and cfg are its arguments).  The temporal history is dropped at every refit --
    the reprojection knows camera motion, not object motion -- so every frame is a first frame to the temporal stage.  A generator of
    (index, result, features, picture, stats), as render_interactive's.  The scene object itself is not changed.  Everything that can be
    checked without a device is checked here.
    track_motion=True switches motion tracking on before the upload (Renderer.track_motion; switched back off at the end) and uses the
    *_moving chained call: the history survives the refits, every pixel reprojected along the motion of the triangle it sees.
    variance_guided=True (with denoise=True) uses Renderer.denoise_temporal_vg in the chained call's place, as render_interactive does;
    track_motion=True then selects its moving stage."""
    if not isinstance(track_motion, (bool, np.bool_)):
        raise TypeError("render_animated: track_motion must be a bool, got %r" % (track_motion,))
    min_len, cfg = _variance_guided_cfg("render_animated", variance_guided, denoise, cfg)
    if not isinstance(cam, B.CameraData):
        raise TypeError("render_animated: cam is no CameraData (camera_init makes one), got %r" % type(cam).__name__)
    frames = list(frames)
    if not frames:
        raise ValueError("render_animated: no frame (give at least one vertex array)")
    for k, v in enumerate(frames):
        if isinstance(v, np.ndarray):
            frames[k] = refit_vertices("render_animated: frames[%d]" % k, v)
    sched = progressive_schedule([spp])
    tkw = dict(temporal or {})
    _temporal_cfg("render_animated", tkw)
    dkw = None
    if despeckle is not None:
        dkw = dict(despeckle)
        unknown = sorted(set(dkw) - set(_DESPECKLE_KEYS))
        if unknown:
            raise TypeError("render_animated: unknown despeckle keyword(s) %s (%s)" % (", ".join(unknown), ", ".join(_DESPECKLE_KEYS)))
        despeckle_config(**dkw)
    vg = None if min_len is None else dict(cfg, min_len=min_len)      # (checked above)
    if vg is not None:
        pass
    elif denoise:
        denoise_config(**cfg)
    elif cfg:
        raise TypeError("render_animated: %s given with denoise=False, which runs no denoiser" % ", ".join(sorted(cfg)))
    elif dkw is not None:
        raise ValueError("render_animated: despeckle given with denoise=False: the firefly filter runs in the denoiser's chain")
    if track_motion:
        return _animated_frames_tracked(scene, cam, frames, width, height, sched[0], bounce_limit, seed, device, renderer, bool(denoise), dkw, tkw, cfg, vg)
    return _animated_frames(scene, cam, frames, width, height, sched[0], bounce_limit, seed, device, renderer, bool(denoise), dkw, tkw, cfg, vg)


def _animated_frames_tracked(scene, cam, frames, width, height, spp, bounce_limit, seed, device, renderer, denoise, despeckle, temporal, cfg, vg=None):
    r = renderer or Renderer(device)
    try:
        r.track_motion(True)      # (before the upload: the upload is what makes the vertices known)
        with _image_session(scene, cam, width, height, spp, bounce_limit, seed, device, r):
            for k, v in enumerate(frames):
                r.refit(v)      # (invalidates the accumulation; the temporal history stays)
                r.accum_reset_features()
                r.render_chunk_accum(width, height, spp)
                r.scatter_tiles()
                if vg is not None:
                    picture = r.denoise_temporal_vg(width, height, temporal, despeckle, moving=True, **vg)
                else:
                    picture = (r.denoise_temporal_moving(width, height, temporal, despeckle, **cfg) if denoise
                               else r.temporal_moving(width, height, **temporal))
                yield k, _collect(r, width, height), r.read_features(width, height), picture, picture["stats"]
    finally:
        if r._h:
            r.track_motion(False)
        if renderer is None:
            r.close()


def _animated_frames(scene, cam, frames, width, height, spp, bounce_limit, seed, device, renderer, denoise, despeckle, temporal, cfg, vg=None):
    with _image_session(scene, cam, width, height, spp, bounce_limit, seed, device, renderer) as r:
        for k, v in enumerate(frames):
            r.refit(v)      # (invalidates the accumulation and drops the temporal history, as an upload does)
            r.accum_reset_features()
            r.render_chunk_accum(width, height, spp)
            r.scatter_tiles()
            if vg is not None:
                picture = r.denoise_temporal_vg(width, height, temporal, despeckle, **vg)
            else:
                picture = r.denoise_temporal(width, height, temporal, despeckle, **cfg) if denoise else r.temporal(width, height, **temporal)
            yield k, _collect(r, width, height), r.read_features(width, height), picture, picture["stats"]


MAX_DENOISE_LEVELS = 8


def denoise_config(levels=5, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1):
    """srt_denoise from Python numbers, checked as the library checks it (ValueError): levels a whole number in [0, 8]; every sigma > 0
    in float32 and not NaN (inf switches its term off).  sigma_color is the level-0 width in XYZ units and halves with every level;
    sigma_depth is relative (a fraction of the larger of two hit distances).  The defaults are starting values, not measurements."""
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 0 <= levels <= MAX_DENOISE_LEVELS:
        raise ValueError("denoise: levels must be a whole number in [0, %d], got %r" % (MAX_DENOISE_LEVELS, levels))
    sig = []
    for name, v in (("sigma_color", sigma_color), ("sigma_normal", sigma_normal), ("sigma_albedo", sigma_albedo), ("sigma_depth", sigma_depth)):
        try:
            if isinstance(v, bool):
                raise TypeError
            with np.errstate(over="ignore"):          # (a value beyond float32 becomes inf, which is allowed)
                f = float(np.float32(v))
        except (TypeError, ValueError):
            raise ValueError("denoise: %s must be a number, got %r" % (name, v))
        if not f > 0.0:
            raise ValueError("denoise: %s must be > 0 in float32 (inf switches the term off), got %r" % (name, v))
        sig.append(f)
    return B.Denoise(int(levels), sig[0], sig[1], sig[2], sig[3], (C.c_uint32 * 3)(0, 0, 0))


def _denoise_number(name, v):
    """v as a float32 held in a Python float (a value beyond float32 becomes inf); ValueError for what is no number"""
    try:
        if isinstance(v, bool):
            raise TypeError
        with np.errstate(over="ignore"):
            return float(np.float32(v))
    except (TypeError, ValueError):
        raise ValueError("denoise: %s must be a number, got %r" % (name, v))


def denoise_vg_config(levels=5, sigma_variance=2.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1, variance_floor=1e-8):
    """srt_denoise_vg from Python numbers, checked as the library checks it (ValueError): levels a whole number in [0, 8]; sigma_variance
    > 0 and finite in float32 -- the luminance term's width in standard deviations of the pixel's estimated noise; the three guide sigmas
    as in denoise_config (inf switches a guide off); variance_floor > 0 in float32, in squared XYZ units -- the luminance term's width
    where the estimate is 0 (inf switches the term off).  sigma_variance and variance_floor are starting values, not tuned, like the
    other defaults."""
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 0 <= levels <= MAX_DENOISE_LEVELS:
        raise ValueError("denoise: levels must be a whole number in [0, %d], got %r" % (MAX_DENOISE_LEVELS, levels))
    sv = _denoise_number("sigma_variance", sigma_variance)
    if not sv > 0.0 or sv == float("inf"):
        raise ValueError("denoise: sigma_variance must be > 0 and finite in float32, got %r" % (sigma_variance,))
    sig = []
    for name, v in (("sigma_normal", sigma_normal), ("sigma_albedo", sigma_albedo), ("sigma_depth", sigma_depth)):
        f = _denoise_number(name, v)
        if not f > 0.0:
            raise ValueError("denoise: %s must be > 0 in float32 (inf switches the term off), got %r" % (name, v))
        sig.append(f)
    vf = _denoise_number("variance_floor", variance_floor)
    if not vf > 0.0:
        raise ValueError("denoise: variance_floor must be > 0 in float32 (inf switches the luminance term off), got %r" % (variance_floor,))
    return B.DenoiseVG(int(levels), sv, sig[0], sig[1], sig[2], vf, (C.c_uint32 * 2)(0, 0))


def render_denoised(scene, cam, width, height, passes, bounce_limit, seed=1984, device=0, renderer=None, variance_guided=False, **cfg):
    """render_features with the denoiser behind every pass: a generator of (spp_total, result, features, denoised), `denoised` the dict
    of Renderer.denoise (cfg: the keywords of denoise_config) for the samples held so far -- with variance_guided=True the dict of
    Renderer.denoise_vg (cfg: the keywords of denoise_vg_config).  The denoiser only reads the accumulation, so result and features are
    render_features' bit for bit.  Schedule and cfg are checked here, before any device is touched."""
    sched = progressive_schedule(passes)
    if variance_guided:
        denoise_vg_config(**cfg)
    else:
        denoise_config(**cfg)
    return _denoised_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, cfg, bool(variance_guided))


def _denoised_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, cfg, variance_guided=False):
    with _image_session(scene, cam, width, height, sum(sched), bounce_limit, seed, device, renderer) as r:
        r.accum_reset_features()
        for spp_add in sched:
            r.render_chunk_accum(width, height, spp_add)
            r.scatter_tiles()
            den = r.denoise_vg(width, height, **cfg) if variance_guided else r.denoise(width, height, **cfg)
            yield r.accum_samples, _collect(r, width, height), r.read_features(width, height), den


def render_developed_denoised(scene, cam, width, height, passes, bounce_limit, response=None, filter=None, scale=None, seed=1984, device=0, renderer=None, **cfg):
    """render_developed and render_denoised in one spectral featured accumulation: a generator of (spp_total, result, developed,
    denoised) after every pass -- `developed` the (H, W, K) planes of Renderer.develop_spectral (sums over the samples held so far),
    `denoised` the dict(dev, xyz) of Renderer.denoise_developed for the same curves (means, filtered; cfg: the keywords of
    denoise_config).  response=None: the colour-matching rows at scale=None, the float32 470/7, so that `developed` holds XYZ sums;
    else scale=None is 1.  Neither call changes the accumulation, so result is render_spectral's bit for bit.  Schedule, curves,
    filter, scale and cfg are checked here, before any device is touched."""
    sched = progressive_schedule(passes)
    resp = sensor_response(cie_response() if response is None else response, filter)
    s = (CIE_SCALE if response is None else 1.0) if scale is None else _develop_scale(scale)
    denoise_config(**cfg)
    return _developed_denoised_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, resp, s, cfg)


def _developed_denoised_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, resp, scale, cfg):
    with _image_session(scene, cam, width, height, sum(sched), bounce_limit, seed, device, renderer) as r:
        r.accum_reset_spectral_features()
        for spp_add in sched:
            r.render_chunk_accum(width, height, spp_add)
            r.scatter_tiles()
            out = _collect(r, width, height)
            dev = r.develop_spectral(width, height, resp, scale)
            yield r.accum_samples, out, dev, r.denoise_developed(width, height, resp, scale, **cfg)


ADAPTIVE_DENOISE_VARIANCE = ("measured", "spatial", None)


def render_adaptive_denoised(scene, cam, width, height, bounce_limit, rel_tol, abs_tol=0.0, min_spp=16, step=16, max_spp=1024, variance="measured",
                             seed=1984, device=0, renderer=None, **cfg):
    """render_adaptive on an adaptive featured accumulation with a denoiser behind every pass: a generator of (spp_total, active_pixels,
    result, features, denoised).  result is render_adaptive's bit for bit (`samples` included), features the raw sums of read_features
    (a pixel's row belongs to the samples that pixel holds: feature_means(features, result["samples"].reshape(height, width))), and
    denoised the dict of Renderer.denoise_mv for variance="measured" (guided by the variance the sampler measured), of
    Renderer.denoise_vg for "spatial" (cfg: the keywords of denoise_vg_config for both) or of Renderer.denoise for None (the plain
    filter; cfg: the keywords of denoise_config).  Every denoiser divides a pixel by its own sample count.  Stops as render_adaptive
    stops.  The arguments are checked here, before any device is touched."""
    if variance not in ADAPTIVE_DENOISE_VARIANCE:
        raise ValueError("render_adaptive_denoised: variance must be 'measured', 'spatial' or None, got %r" % (variance,))
    acfg = adaptive_config(rel_tol, abs_tol, min_spp)
    sched = adaptive_schedule(min_spp, step, max_spp)
    if variance is None:
        denoise_config(**cfg)
    else:
        denoise_vg_config(**cfg)
    return _adaptive_denoised_passes(scene, cam, width, height, bounce_limit, acfg, sched, seed, device, renderer, variance, cfg)


def _adaptive_denoised_passes(scene, cam, width, height, bounce_limit, acfg, sched, seed, device, renderer, variance, cfg):
    with _image_session(scene, cam, width, height, sum(sched), bounce_limit, seed, device, renderer) as r:
        r._ck(B.lib().srt_accum_reset_adaptive_features(r._h, C.byref(acfg)))      # (after the session has set the planes)
        for spp_add in sched:
            r.render_chunk_accum(width, height, spp_add)
            r.scatter_tiles()
            active = r.accum_active
            out = _collect(r, width, height)
            out["samples"] = r.accum_stats(width, height)["samples"]
            den = r.denoise_mv(width, height, **cfg) if variance == "measured" else r.denoise_vg(width, height, **cfg) if variance == "spatial" else r.denoise(width, height, **cfg)
            yield r.accum_samples, active, out, r.read_features(width, height), den
            if active == 0:
                break


def render_adaptive_spectral(scene, cam, width, height, bounce_limit, rel_tol, abs_tol=0.0, min_spp=16, step=16, max_spp=1024, features=False,
                             response=None, filter=None, scale=None, seed=1984, device=0, renderer=None, **cfg):
    """render_adaptive on an adaptive spectral accumulation: a generator of (spp_total, active_pixels, result, radiance) after every pass
    -- result is render_adaptive's bit for bit (`samples` included) and radiance spectral_radiance(film, result["samples"]), (H, W, 95):
    every pixel's film divided by the samples that pixel holds.  features=True runs the adaptive spectral featured accumulation and yields
    two more items, `developed` (Renderer.develop_spectral's (H, W, K) sums) and `denoised` (the dict of Renderer.denoise_developed;
    response, filter and scale as render_developed_denoised, cfg: the keywords of denoise_config).  Without features there is nothing to
    develop for: response, filter, scale and cfg must be left alone.  Stops as render_adaptive stops.  The arguments are checked here,
    before any device is touched."""
    acfg = adaptive_config(rel_tol, abs_tol, min_spp)
    sched = adaptive_schedule(min_spp, step, max_spp)
    if not isinstance(features, (bool, np.bool_)):
        raise ValueError("render_adaptive_spectral: features must be True or False, got %r" % (features,))
    resp, s = None, None
    if features:
        resp = sensor_response(cie_response() if response is None else response, filter)
        s = (CIE_SCALE if response is None else 1.0) if scale is None else _develop_scale(scale)
        denoise_config(**cfg)
    elif response is not None or filter is not None or scale is not None or cfg:
        raise ValueError("render_adaptive_spectral: response, filter, scale and the denoiser's keywords need features=True")
    return _adaptive_spectral_passes(scene, cam, width, height, bounce_limit, acfg, sched, seed, device, renderer, bool(features), resp, s, cfg)


def _adaptive_spectral_passes(scene, cam, width, height, bounce_limit, acfg, sched, seed, device, renderer, features, resp, scale, cfg):
    with _image_session(scene, cam, width, height, sum(sched), bounce_limit, seed, device, renderer) as r:
        reset = B.lib().srt_accum_reset_adaptive_spectral_features if features else B.lib().srt_accum_reset_adaptive_spectral
        r._ck(reset(r._h, C.byref(acfg)))      # (after the session has set the planes)
        for spp_add in sched:
            r.render_chunk_accum(width, height, spp_add)
            r.scatter_tiles()
            active = r.accum_active
            out = _collect(r, width, height)
            out["samples"] = r.accum_stats(width, height)["samples"]
            radiance = spectral_radiance(r.read_spectral(width, height), out["samples"].reshape(height, width))
            if features:
                dev = r.develop_spectral(width, height, resp, scale)
                yield r.accum_samples, active, out, radiance, dev, r.denoise_developed(width, height, resp, scale, **cfg)
            else:
                yield r.accum_samples, active, out, radiance
            if active == 0:
                break


PRESENT_SOURCES = tuple(B.PRESENT_SOURCES)      # "accum", "denoise", "denoise_vg", "denoise_mv", "develop"
_DENOISE_KEYS = ("levels", "sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth")
_DENOISE_VG_KEYS = ("levels", "sigma_variance", "sigma_normal", "sigma_albedo", "sigma_depth", "variance_floor")
_DEVELOP_KEYS = ("response", "filter", "scale")
_PRESENT_STAGE_KEYS = {"accum": (), "denoise": _DENOISE_KEYS, "denoise_vg": _DENOISE_VG_KEYS, "denoise_mv": _DENOISE_VG_KEYS, "develop": _DEVELOP_KEYS}


def present_config(source="accum", gain=None, **cfg):
    """srt_present_cfg from Python values, checked as the library checks it, before any device is touched.  source: "accum" (the sums),
    "denoise", "denoise_vg", "denoise_mv" (the three filters) or "develop" (the film through three curves taken as X, Y, Z).  gain None:
    the exposure is metered on the source picture; else the gain.  cfg is told apart by name: the keywords of meter_config (only without a
    gain), of tone_config (curve, white), of denoise_config / denoise_vg_config (only on the source that runs that filter) and response,
    filter, scale as Renderer.develop_spectral_srgb takes them (only on "develop").  TypeError for a name that is none of them; ValueError
    for an unknown source, meter keywords with an explicit gain, a stage's keywords on a source that does not run it, and every value its
    own config function refuses."""
    if not isinstance(source, str) or source not in B.PRESENT_SOURCES:
        raise ValueError("present: source must be one of %s, got %r" % (", ".join(PRESENT_SOURCES), source))
    known = set(_METER_KEYS) | set(_TONE_KEYS) | set(_DENOISE_KEYS) | set(_DENOISE_VG_KEYS) | set(_DEVELOP_KEYS)
    unknown = sorted(set(cfg) - known)
    if unknown:
        raise TypeError("present: unknown keyword(s) %s" % ", ".join(unknown))
    mcfg = {k: v for k, v in cfg.items() if k in _METER_KEYS}
    tcfg = {k: v for k, v in cfg.items() if k in _TONE_KEYS}
    scfg = {k: v for k, v in cfg.items() if k not in _METER_KEYS and k not in _TONE_KEYS}
    if gain is not None and mcfg:
        raise ValueError("present: %s given with an explicit gain, which is not metered" % ", ".join(sorted(mcfg)))
    stray = sorted(set(scfg) - set(_PRESENT_STAGE_KEYS[source]))
    if stray:
        raise ValueError("present: %s given with source %r, which does not run that stage" % (", ".join(stray), source))
    p = B.PresentCfg()
    p.source = B.PRESENT_SOURCES[source]
    p.metered = 1 if gain is None else 0
    p.meter = meter_config(**mcfg)
    p.tone = tone_config(gain=1.0 if gain is None else gain, **tcfg)
    p.denoise = denoise_config(**(scfg if source == "denoise" else {}))
    p.denoise_vg = denoise_vg_config(**(scfg if source in ("denoise_vg", "denoise_mv") else {}))
    p.scale = CIE_SCALE
    if source == "develop":
        response, filter = scfg.get("response"), scfg.get("filter")
        if response is not None or filter is not None:
            resp = sensor_response(cie_response() if response is None else response, filter)
            if resp.shape[0] != 3:
                raise ValueError("present: needs three response curves (taken as X, Y, Z), got %d" % resp.shape[0])
            p._response = resp      # (the struct only points at the curves)
            p.response3 = B.fptr(resp)
        if scfg.get("scale") is not None:
            p.scale = _develop_scale(scfg["scale"])
    return p


def render_presented(scene, cam, width, height, passes, bounce_limit, source="accum", gain=None, seed=1984, device=0, renderer=None,
                     rel_tol=0.02, abs_tol=0.0, min_spp=16, **cfg):
    """render_progressive with the picture presented on the device behind every pass: a generator of (spp_total, result, presented) --
    `result` with the keys of render_image, `presented` the dict of Renderer.present(width, height, source, gain, **cfg).  The
    accumulation is the kind the source needs: plain for "accum", featured for "denoise" and "denoise_vg", adaptive featured for
    "denoise_mv" (rel_tol, abs_tol, min_spp: its stopping rule, read by no other source; the first pass must hold at least 2 samples),
    spectral for "develop".  Presenting only reads the accumulation, so result is that kind's own generator's bit for bit.  Schedule and
    cfg are checked here, before any device is touched."""
    sched = progressive_schedule(passes)
    present_config(source, gain, **cfg)
    acfg = adaptive_config(rel_tol, abs_tol, min_spp) if source == "denoise_mv" else None
    return _presented_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, source, gain, acfg, cfg)


def _presented_passes(scene, cam, width, height, sched, bounce_limit, seed, device, renderer, source, gain, acfg, cfg):
    with _image_session(scene, cam, width, height, sum(sched), bounce_limit, seed, device, renderer) as r:
        if source == "accum":
            r.accum_reset()
        elif source == "develop":
            r.accum_reset_spectral()
        elif source == "denoise_mv":
            r._ck(B.lib().srt_accum_reset_adaptive_features(r._h, C.byref(acfg)))      # (after the session has set the planes)
        else:
            r.accum_reset_features()
        for spp_add in sched:
            r.render_chunk_accum(width, height, spp_add)
            r.scatter_tiles()
            out = _collect(r, width, height)
            yield r.accum_samples, out, r.present(width, height, source, gain, **cfg)
