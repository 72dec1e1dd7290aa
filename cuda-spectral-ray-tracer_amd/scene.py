"""Host-side scene handle (srt_scene): replaces scene_manager's device-heap world (scene/scene.cuh:103-176)."""
import ctypes as C

import numpy as np

from . import binding as B


def camera_init(width, height, vfov, lookfrom, lookat, vup=(0, 1, 0), defocus_angle=0.0, focus_dist=10.0):
    """camera::initialize (rendering/camera.cu:7-58) -> camera_data (rendering/rendering.cuh:28-36)."""
    cam = B.CameraData()
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    B.check(B.lib().srt_camera_init(int(width), int(height), float(vfov), f3(lookfrom), f3(lookat), f3(vup),
                                    float(defocus_angle), float(focus_dist), C.byref(cam)))
    return cam


def refit_vertices(who, vertices):
    """the (n, 3, 3) float32 vertex array of a refit, C-contiguous; anything else is refused here, before any library call"""
    if not isinstance(vertices, np.ndarray):
        raise TypeError("%s: vertices must be a numpy array (n_tris, 3, 3) float32, got %r" % (who, type(vertices).__name__))
    if vertices.dtype != np.float32:
        raise TypeError("%s: vertices must be float32, got %s" % (who, vertices.dtype))
    if vertices.ndim != 3 or vertices.shape[1:] != (3, 3) or vertices.shape[0] == 0:
        raise ValueError("%s: vertices must have shape (n_tris, 3, 3) with n_tris >= 1, got %r" % (who, vertices.shape))
    return np.ascontiguousarray(vertices)


def ray_segments(who, segments):
    """the (n, 7) float32 segment array of the ray-tuned tree calls -- origin, direction, t_end --, C-contiguous; n may be 0"""
    seg = np.asarray(segments, np.float32)
    if seg.size == 0:
        return np.zeros((0, 7), np.float32)
    if seg.ndim != 2 or seg.shape[1] != 7:
        raise ValueError("%s: segments must have shape (n, 7), got %r" % (who, seg.shape))
    return np.ascontiguousarray(seg)


class Scene:
    def __init__(self, handle):
        if not handle:
            raise B.SrtError(-1, (B.lib().srt_last_error(None) or b"").decode())
        self._h = C.c_void_p(handle)

    @classmethod
    def builtin(cls, scene_id, seed=0):
        return cls(B.lib().srt_scene_builtin(int(scene_id), int(seed)))

    @classmethod
    def from_arrays(cls, tris, materials, background):
        """tris: ctypes array of TriIn; materials: ctypes array of Material; background: 95 floats."""
        s = cls(B.lib().srt_scene_create())
        B.check(B.lib().srt_scene_set_triangles(s._h, tris, len(tris)))
        B.check(B.lib().srt_scene_set_materials(s._h, materials, len(materials)))
        bg = np.ascontiguousarray(background, dtype=np.float32)
        assert bg.shape == (B.N_CIE,)
        B.check(B.lib().srt_scene_set_background(s._h, B.fptr(bg)))
        return s

    def close(self):
        if self._h:
            B.lib().srt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def n_tris(self):
        return B.lib().srt_scene_tri_count(self._h)

    @property
    def n_materials(self):
        return B.lib().srt_scene_material_count(self._h)

    def triangles(self):
        arr = (B.TriIn * self.n_tris)()
        B.check(B.lib().srt_scene_get_triangles(self._h, arr))
        return arr

    def materials(self):
        arr = (B.Material * self.n_materials)()
        B.check(B.lib().srt_scene_get_materials(self._h, arr))
        return arr

    def background(self):
        bg = np.zeros(B.N_CIE, np.float32)
        B.check(B.lib().srt_scene_get_background(self._h, B.fptr(bg)))
        return bg

    def tri_records(self):
        out = np.zeros((self.n_tris, 12), np.float32)
        B.check(B.lib().srt_scene_get_tri_records(self._h, B.fptr(out)))
        return out

    def build_bvh(self, mode=B.BVH_REFERENCE, seed=1984):
        B.check(B.lib().srt_scene_build_bvh(self._h, int(mode), int(seed)))
        return self

    def refit(self, vertices):
        """new vertices on the built topology (srt_scene_refit): vertices (n_tris, 3, 3) float32, v0 v1 v2 of every triangle.  Triangle
        products, node boxes and depth are recomputed; topology, child order, materials and the stored aa_plane stay.  Upload the scene
        afterwards, or give the same vertices to Renderer.refit on a renderer that holds it."""
        v = refit_vertices("Scene.refit", vertices)
        B.check(B.lib().srt_scene_refit(self._h, B.fptr(v), v.shape[0]))
        return self

    def vertices(self):
        """the triangles' vertices as the (n_tris, 3, 3) float32 array refit() takes (a copy)"""
        t = self.triangles()
        words = np.frombuffer(t, np.float32).reshape(len(t), C.sizeof(B.TriIn) // 4)      # 9 vertex floats, then mat_index and aa_plane
        return np.ascontiguousarray(words[:, :9]).reshape(len(t), 3, 3)

    def refit_schedule(self):
        """the records of every height a device refit of this scene handles in one launch each, bottom up (srt_scene_refit_schedule):
        a uint32 array, empty when the root is a leaf"""
        n = C.c_uint32()
        B.check(B.lib().srt_scene_refit_schedule(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint32)
        if out.size:
            B.check(B.lib().srt_scene_refit_schedule(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(n)))
        return out

    def optimise_bvh(self, passes=3):
        """insertion-based topology optimisation of the built tree (srt_scene_optimise_bvh): for throughput-bound launches"""
        B.check(B.lib().srt_scene_optimise_bvh(self._h, passes))
        return self

    def optimise_bvh_for_rays(self, segments, passes=3):
        """srt_scene_optimise_bvh against a sample of a frame's closest-hit queries (srt_scene_optimise_bvh_for_rays): segments (n, 7)
        float32 -- origin, direction, t_end -- as Renderer.collect_ray_segments returns them; an empty array is optimise_bvh"""
        seg = ray_segments("Scene.optimise_bvh_for_rays", segments)
        B.check(B.lib().srt_scene_optimise_bvh_for_rays(self._h, passes, B.fptr(seg), seg.shape[0]))
        return self

    def bvh_ray_cost(self, segments):
        """the objective of optimise_bvh_for_rays for the built tree and a sample (srt_scene_bvh_ray_cost)"""
        seg = ray_segments("Scene.bvh_ray_cost", segments)
        cost = C.c_double()
        B.check(B.lib().srt_scene_bvh_ray_cost(self._h, B.fptr(seg), seg.shape[0], C.byref(cost)))
        return cost.value

    def order_children(self, eye):
        """Re-order every node's children for a viewpoint (nearer child first); upload the scene again afterwards."""
        e = (C.c_float * 3)(*[float(x) for x in eye])
        B.check(B.lib().srt_scene_order_children(self._h, e))
        return self

    @property
    def n_nodes(self):
        return B.lib().srt_scene_node_count(self._h)

    @property
    def is_paired(self):
        """every internal node has two leaf children or none (SAH builder, even triangle count): the launch uses the PAIRED kernel variant"""
        return bool(B.lib().srt_scene_is_paired(self._h))

    @property
    def bvh_depth(self):
        return B.lib().srt_scene_bvh_depth(self._h)

    def bvh(self):
        n = self.n_nodes
        left, right, prim = (np.zeros(n, np.int32) for _ in range(3))
        boxes = np.zeros((n, 6), np.float32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        B.check(B.lib().srt_scene_get_bvh(self._h, ip(left), ip(right), ip(prim), B.fptr(boxes)))
        return left, right, prim, boxes

    def default_camera(self, width, height):
        cam = B.CameraData()
        B.check(B.lib().srt_scene_default_camera(self._h, int(width), int(height), C.byref(cam)))
        return cam
