"""Host-side mirror of the reference's Engine API for the render path, over the C ABI.

The reference's host is C# (`Engine/RTRenderer.cs`, `Engine/Scene.cs`, `Engine/SceneManager.cs`,
`Engine/Camera.cs`); there is no .NET toolchain in this image, so this module plays the
C# host's role from Python with the same class / method names and argument meaning:

    Scene.AddSphere / BuildSphereInstance / LoadObjInstance* / RebuildTLAS / BuildDefaultScene
    SceneManager.Commit  ->  RTRenderer.commit(scene)      (Scene.UploadAll, Scene.cs:258-279)
    RTRenderer.RenderDirectToPbo(pbo, w, h, frame, dt) -> RTRenderer.render_direct(w, h, frame, dt); its host half is FrameHost
    RTRenderer.SetSunParams, Camera.CreateCamera / look-at ctor / Translate

(* the array-append half; the OBJ file parser is out of scope.)

Everything computed here is plumbing: the scene builders, camera math and the two kernels
all live in libhip_raytrace.so (csrc/).  There is NO fallback: if the library or a GPU is
missing, constructing RTRenderer raises.
"""
import ctypes as C
import os
import random

import numpy as np

from . import _types as T

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HRT_LIB") or os.path.join(_HERE, "csrc", "libhip_raytrace.so")   # HRT_LIB: A/B builds of the same library
_LIB = None
_HOOKS = None
HOOKS_LIB_PATH = os.environ.get("HRT_HOOKS_LIB") or os.path.join(_HERE, "csrc", "libhip_raytrace_test.so")


class HrtError(RuntimeError):
    """A C-ABI call returned a negative hrt_status."""

    def __init__(self, code, msg):
        super().__init__("hip_raytrace error %d: %s" % (code, msg))
        self.code = code


def _load(path, hooks=False):
    if not os.path.exists(path):
        raise ImportError("%s is not built. Run __graft_entry__.build(); there is no CPU fallback for the render path." % path)
    L = C.CDLL(path)
    L.hrt_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
    L.hrt_destroy.argtypes = [C.c_void_p]
    L.hrt_destroy.restype = None
    L.hrt_last_error.argtypes = [C.c_void_p]
    L.hrt_last_error.restype = C.c_char_p
    L.hrt_scene_upload.argtypes = [C.c_void_p, C.POINTER(T.SceneDesc)]
    L.hrt_scene_update_instances.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(T.BvhUpdateStats)]
    L.hrt_scene_update_positions.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(T.BvhUpdateStats)]
    L.hrt_scene_update_spheres.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(T.BvhUpdateStats)]
    L.hrt_scene_download_array.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.hrt_scene_download_tlas.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                          C.POINTER(C.c_int64)]
    L.hrt_render_frame.argtypes = [C.c_void_p, C.POINTER(T.FrameParams), C.POINTER(T.RenderOpts), C.POINTER(T.Outputs), C.POINTER(T.Stats)]
    L.hrt_render_progressive.argtypes = [C.c_void_p, C.POINTER(T.FrameParams), C.POINTER(T.RenderOpts), C.c_int32, C.POINTER(T.Outputs),
                                         C.POINTER(T.Stats)]
    L.hrt_synchronize.argtypes = [C.c_void_p, C.POINTER(T.Stats)]
    L.hrt_present.argtypes = [C.c_void_p, C.POINTER(T.PresentParams), C.c_void_p]
    L.hrt_present_time.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.hrt_motion_vectors.argtypes = [C.c_void_p, C.POINTER(T.Camera), C.c_void_p, C.c_int32, C.POINTER(C.c_float)]
    L.hrt_denoise.argtypes = [C.c_void_p, C.POINTER(T.DenoiseParams), C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    L.hrt_denoised_buffers.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.hrt_denoise_temporal.argtypes = [C.c_void_p, C.POINTER(T.DenoiseTemporalParams), C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    L.hrt_denoise_history.argtypes = [C.c_void_p, C.POINTER(T.DenoiseHistoryViews)]
    L.hrt_denoise_history_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.hrt_device_buffers.argtypes = [C.c_void_p, C.c_int, C.POINTER(T.DeviceViews)]
    L.hrt_reset_history.argtypes = [C.c_void_p]
    L.hrt_frame_times.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.hrt_host_register.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.hrt_host_unregister.argtypes = [C.c_void_p, C.c_void_p]
    L.hrt_set_workspace_limit.argtypes = [C.c_void_p, C.c_int64]
    L.hrt_trace_rays.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(C.c_float)]
    L.hrt_trace_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                 C.POINTER(C.c_float)]
    L.hrt_trace_paths.argtypes = [C.c_void_p, C.POINTER(T.FrameParams), C.c_uint32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                  C.c_int32, C.POINTER(C.c_float)]
    L.hrt_device_count.restype = C.c_int
    L.hrt_version.restype = C.c_char_p
    L.hrth_scene_new.restype = C.c_void_p
    L.hrth_scene_free.argtypes = [C.c_void_p]
    L.hrth_scene_free.restype = None
    L.hrth_scene_clear.argtypes = [C.c_void_p]
    L.hrth_scene_build_default.argtypes = [C.c_void_p]
    L.hrth_scene_add_texture.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.hrth_scene_add_sphere.argtypes = [C.c_void_p, C.POINTER(T.Sphere)]
    L.hrth_scene_build_sphere_instance.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(T.Affine3x4)]
    L.hrth_scene_load_mesh_instance.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(T.Affine3x4)]
    L.hrth_mesh_load_obj.argtypes = [C.c_char_p, C.c_float, C.c_int, C.POINTER(C.c_void_p)]
    L.hrth_mesh_get.argtypes = [C.c_void_p, C.POINTER(T.MeshDesc)]
    L.hrth_mesh_free.argtypes = [C.c_void_p]
    L.hrth_mesh_free.restype = None
    L.hrth_mesh_material_name.argtypes = [C.c_void_p, C.c_int]
    L.hrth_mesh_material_name.restype = C.c_char_p
    L.hrth_mesh_texture_path.argtypes = [C.c_void_p, C.c_int]
    L.hrth_mesh_texture_path.restype = C.c_char_p
    L.hrth_image_load.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_uint8))]
    L.hrth_image_free.argtypes = [C.POINTER(C.c_uint8)]
    L.hrth_image_free.restype = None
    L.hrth_scene_load_obj_instance.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(T.Affine3x4), C.c_float]
    L.hrth_last_error.restype = C.c_char_p
    L.hrth_scene_rebuild_tlas.argtypes = [C.c_void_p]
    L.hrth_scene_set_instance_transform.argtypes = [C.c_void_p, C.c_int, C.POINTER(T.Affine3x4)]
    L.hrth_scene_get_desc.argtypes = [C.c_void_p, C.POINTER(T.SceneDesc)]
    L.hrth_camera_create.argtypes = [C.c_int, C.c_int, C.c_float, C.POINTER(T.Camera)]
    L.hrth_camera_lookat.argtypes = [C.POINTER(C.c_float)] * 3 + [C.c_float, C.c_float, C.c_float, C.POINTER(T.Camera)]
    L.hrth_camera_translate.argtypes = [C.POINTER(T.Camera), C.POINTER(C.c_float)]
    L.hrth_camera_bake.argtypes = [C.POINTER(T.Camera), C.c_int, C.c_int]
    L.hrth_sun_dir.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_float)]
    if hooks:       # include/hrt_test_hooks.h: only in libhip_raytrace_test.so
        L.hrt_math_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hrt_math_exhaustive.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        L.hrt_debug_set_treelet_limits.argtypes = [C.c_int, C.c_int, C.c_int]
        L.hrt_debug_treelet_count.argtypes = [C.c_void_p]
        L.hrt_debug_treelets.argtypes = [C.POINTER(T.SceneDesc), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_int64)]
    return L


def lib():
    """Loads libhip_raytrace.so, the shipped library (built by `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _LIB
    if _LIB is None:
        _LIB = _load(LIB_PATH)
    return _LIB


def hooks():
    """Loads libhip_raytrace_test.so: the same sources compiled with -DHRT_TEST_HOOKS (include/hrt_test_hooks.h).  Test suite only;
    a renderer that needs a hook is created with RTRenderer(..., library=hooks())."""
    global _HOOKS
    if _HOOKS is None:
        _HOOKS = _load(HOOKS_LIB_PATH, hooks=True)
    return _HOOKS


def _fv(v):
    return (C.c_float * 3)(*[float(x) for x in v])


# ------------------------------------------------------------------ Camera (Engine/Camera.cs)
def create_camera(width, height, fov_degrees):
    """Camera.CreateCamera (Camera.cs:19-47)."""
    c = T.Camera()
    lib().hrth_camera_create(width, height, fov_degrees, C.byref(c))
    return c


def camera_look_at(origin, look_at, up, vfov_degrees, aspect, focus_dist=1.0):
    """new Camera(origin, lookAt, up, vfovDegrees, aspect, focusDist) (Camera.cs:100-119)."""
    c = T.Camera()
    lib().hrth_camera_lookat(_fv(origin), _fv(look_at), _fv(up), vfov_degrees, aspect, focus_dist, C.byref(c))
    return c


def camera_translate(cam, delta):
    """Camera.Translate (Camera.cs:121-126)."""
    lib().hrth_camera_translate(C.byref(cam), _fv(delta))


def bake_camera_derived(cam, pixel_w, pixel_h):
    """RTRenderer.BakeCameraDerived (RTRenderer.cs:241-263)."""
    lib().hrth_camera_bake(C.byref(cam), pixel_w, pixel_h)


def sun_direction(azimuth, elevation):
    o = (C.c_float * 3)()
    lib().hrth_sun_dir(azimuth, elevation, o)
    return [float(v) for v in o]


def copy_camera(cam):
    c = T.Camera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(T.Camera))
    return c


# ------------------------------------------------------------------ mesh container (MeshHost, MeshLoaderOBJ.cs:21-31)
class MeshData:
    """Arrays of one mesh as MeshLoaderOBJ.Load would return them (MeshHost)."""

    def __init__(self, positions, triangles, texcoords, tri_uvs, materials, tri_material_index=None, textures_bgra=()):
        self.positions = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        self.triangles = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        self.texcoords = np.ascontiguousarray(texcoords, dtype=np.float32).reshape(-1, 2)
        self.tri_uvs = np.ascontiguousarray(tri_uvs, dtype=np.int32).reshape(-1, 3)
        self.materials = (T.MaterialRecord * len(materials))(*materials)
        self.n_materials = len(materials)
        self.tri_mat = None if tri_material_index is None else np.ascontiguousarray(tri_material_index, dtype=np.int32)
        self.tex_w = np.array([t.shape[1] for t in textures_bgra], dtype=np.int32)
        self.tex_h = np.array([t.shape[0] for t in textures_bgra], dtype=np.int32)
        self.tex_bytes = np.concatenate([np.ascontiguousarray(t, dtype=np.uint8).reshape(-1) for t in textures_bgra]) \
            if len(textures_bgra) else np.zeros(0, np.uint8)
        self.n_tex = len(textures_bgra)
        assert len(self.tri_uvs) == len(self.triangles)

    def ptrs(self):
        return (self.positions.ctypes.data, len(self.positions), self.triangles.ctypes.data, len(self.triangles),
                self.texcoords.ctypes.data, len(self.texcoords), self.tri_uvs.ctypes.data,
                self.tri_mat.ctypes.data if self.tri_mat is not None else None, len(self.tri_mat) if self.tri_mat is not None else 0,
                C.cast(self.materials, C.c_void_p), self.n_materials,
                self.tex_w.ctypes.data if self.n_tex else None, self.tex_h.ctypes.data if self.n_tex else None,
                self.tex_bytes.ctypes.data if self.n_tex else None, self.n_tex)


class AssetFormatError(ValueError):
    """FormatException / InvalidDataException / EndOfStreamException raised by the reference's loader."""


def _raise_host(rc, what):
    msg = (lib().hrth_last_error() or b"").decode("utf-8", "replace")
    if rc == T.HRTH_ERR_NOT_FOUND:
        raise FileNotFoundError(msg or what)
    if rc == T.HRTH_ERR_FORMAT:
        raise AssetFormatError(msg or what)
    raise ValueError(msg or what)


def load_obj(path, scale=1.0, flip_winding=True):
    """MeshLoaderOBJ.Load (MeshLoaderOBJ.cs:67): OBJ + MTL + textures -> MeshData (material texture indices are local)."""
    h = C.c_void_p()
    rc = lib().hrth_mesh_load_obj(os.fsencode(path), scale, 1 if flip_winding else 0, C.byref(h))
    if rc != 0:
        _raise_host(rc, "load_obj failed")
    try:
        d = T.MeshDesc()
        lib().hrth_mesh_get(h, C.byref(d))

        def arr(ptr, n, dtype, width):
            if n == 0:
                return np.zeros((0, width), dtype)
            return np.frombuffer(C.string_at(ptr, n * width * 4), dtype).reshape(n, width).copy()

        mats = [T.MaterialRecord.from_buffer_copy(C.string_at(C.addressof(d.materials[i]), C.sizeof(T.MaterialRecord))) for i in range(d.n_materials)]
        texs, off = [], 0
        for i in range(d.n_textures):
            w, hgt = d.tex_w[i], d.tex_h[i]
            n = w * hgt * 4
            texs.append(np.frombuffer(C.string_at(C.addressof(d.tex_bgra.contents) + off, n), np.uint8).reshape(hgt, w, 4).copy()
                        if n else np.zeros((hgt, w, 4), np.uint8))
            off += n
        mesh = MeshData(arr(d.positions, d.n_positions, np.float32, 3), arr(d.triangles, d.n_triangles, np.int32, 3),
                        arr(d.texcoords, d.n_texcoords, np.float32, 2), arr(d.tri_uvs, d.n_triangles, np.int32, 3), mats,
                        arr(d.tri_material_index, d.n_tri_material_index, np.int32, 1).reshape(-1), texs)
        mesh.material_names = [(lib().hrth_mesh_material_name(h, i) or b"").decode("utf-8", "replace") for i in range(d.n_materials)]
        mesh.texture_paths = [(lib().hrth_mesh_texture_path(h, i) or b"").decode("utf-8", "replace") for i in range(d.n_textures)]
        return mesh
    finally:
        lib().hrth_mesh_free(h)


def load_image(path):
    """LoadTextureBGRA (MeshLoaderOBJ.cs:456-593): .tga (raw / RLE, 8/24/32 bit), .png (<= 8 bits per sample) or uncompressed .bmp -> (H, W, 4) uint8 BGRA, row 0 = top."""
    w, h, p = C.c_int(), C.c_int(), C.POINTER(C.c_uint8)()
    rc = lib().hrth_image_load(os.fsencode(path), C.byref(w), C.byref(h), C.byref(p))
    if rc != 0:
        _raise_host(rc, "load_image failed")
    try:
        n = w.value * h.value * 4
        return np.frombuffer(C.string_at(p, n), np.uint8).reshape(h.value, w.value, 4).copy()
    finally:
        lib().hrth_image_free(p)


# ------------------------------------------------------------------ Scene (Engine/Scene.cs, host lists + builders)
class Scene:
    def __init__(self):
        self._h = lib().hrth_scene_new()

    def __del__(self):
        try:
            if self._h:
                lib().hrth_scene_free(self._h)
                self._h = None
        except Exception:
            pass

    def build_default_scene(self):
        """Scene.BuildDefaultScene (Scene.cs:83-142)."""
        lib().hrth_scene_build_default(self._h)

    def add_texture(self, rgba):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        h, w = rgba.shape[:2]
        r = lib().hrth_scene_add_texture(self._h, w, h, rgba.ctypes.data)
        if r < 0:
            raise ValueError("add_texture: invalid texture")
        return r

    def add_sphere(self, sphere):
        """Scene.AddSphere (Scene.cs:315-321)."""
        return lib().hrth_scene_add_sphere(self._h, C.byref(sphere))

    def build_sphere_instance(self, sphere_ids, object_to_world=None):
        """Scene.BuildSphereInstance (Scene.cs:323-356); the record is appended to the instance list."""
        ids = list(sphere_ids)
        arr = (C.c_int * len(ids))(*ids)
        m = object_to_world if object_to_world is not None else T.identity_affine()
        r = lib().hrth_scene_build_sphere_instance(self._h, arr, len(ids), C.byref(m))
        if r < 0:
            raise ValueError("build_sphere_instance: invalid sphere ids")
        return r

    def load_mesh_instance(self, mesh, object_to_world=None):
        """Scene.LoadObjInstance after MeshLoaderOBJ.Load (Scene.cs:151-256)."""
        m = object_to_world if object_to_world is not None else T.identity_affine()
        r = lib().hrth_scene_load_mesh_instance(self._h, *mesh.ptrs(), C.byref(m))
        if r < 0:
            raise ValueError("load_mesh_instance: invalid mesh arrays")
        return r

    def load_obj_instance(self, obj_path, object_to_world=None, uniform_scale=1.0):
        """Scene.LoadObjInstance(objPath, objectToWorld, uniformScale) (Scene.cs:144-256)."""
        m = object_to_world if object_to_world is not None else T.identity_affine()
        r = lib().hrth_scene_load_obj_instance(self._h, os.fsencode(obj_path), C.byref(m), uniform_scale)
        if r < 0:
            _raise_host(r, "load_obj_instance failed")
        return r

    def rebuild_tlas(self):
        """Scene.RebuildTLAS (Scene.cs:358-368)."""
        lib().hrth_scene_rebuild_tlas(self._h)

    def set_instance_transform(self, inst_id, xform):
        """Moves an instance of the host scene (records re-derived as at creation); follow with rebuild_tlas() + commit,
        or mirror the move on the device with RTRenderer.update_instances."""
        if lib().hrth_scene_set_instance_transform(self._h, int(inst_id), C.byref(xform)) != 0:
            raise IndexError("instance id out of range")

    def desc(self):
        d = T.SceneDesc()
        lib().hrth_scene_get_desc(self._h, C.byref(d))
        return d

    def arrays(self):
        return T.arrays_from_scene_desc(self.desc())


# ------------------------------------------------------------------ RTRenderer (Engine/RTRenderer.cs)
def _host_fmin(a, b):
    """.NET Math.Min on floats (XMath.Min on the host, include/hrt_math.h hrt_host_fmin): a NaN operand is returned, -0 < +0."""
    if a != a: return a
    if b != b: return b
    if a == b: return a if np.signbit(a) else b
    return a if a < b else b


def _host_fmax(a, b):
    """.NET Math.Max on floats (hrt_host_fmax)."""
    if a != a: return a
    if b != b: return b
    if a == b: return b if np.signbit(a) else a
    return a if a > b else b


TWO_PI_F = np.float32(6.28318530717958647692)                 # RTRenderer.cs:171, a float constant


class FrameHost:
    """The host half of RTRenderer.RenderDirectToPbo (RTRenderer.cs:43-61, 104-236) without a device: the private fields with their
    defaults, the internal size, the camera bake, the float32 sun animation and the FrameParams assembly.  Needs the library's host
    functions (camera, sun direction) but no GPU; RTRenderer inherits it."""

    def __init__(self, width=1280, height=720):
        # private fields of the reference's RTRenderer (RTRenderer.cs:43-61), same defaults; `float` fields are numpy float32
        self.render_scale = np.float32(0.67)
        self.enable_taau = True
        self.enable_reproject = False                             # not a field of the reference: TAAU with camera reprojection (render_direct)
        self.enable_temporal_reuse = 1
        self.enable_spatial_reuse = 1
        self.rng_lock_noise = 1
        self.spp = 2
        self.max_depth = 3                                        # RTRenderer.cs:204, a local constant there
        self.sun_azimuth = np.float32(0.0)
        self.sun_elevation = np.float32(0.9)
        self.sun_speed = np.float32(0.0)
        self.dir_light_radiance = (10.0, 10.0, 10.0)
        self.sky_tint_top = (0.5, 0.7, 1.0)
        self.sky_tint_bottom = (1.0, 1.0, 1.0)
        self.camera = create_camera(max(1, width), max(1, height), 60.0)
        camera_translate(self.camera, (1.0, 0.0, -4.0))           # RTRenderer.cs:78-79
        self.prev_camera = copy_camera(self.camera)
        self.last_made_params = None          # FrameParams of the last make_params (RTRenderer.pick casts its camera's rays)

    def set_sun_params(self, speed_rad_per_sec, elevation_rad):
        """RTRenderer.SetSunParams (RTRenderer.cs:99-103): both are float fields."""
        self.sun_speed = np.float32(speed_rad_per_sec)
        self.sun_elevation = np.float32(elevation_rad)

    def internal_size(self, out_width, out_height, render_scale=None):
        """inW, inH of RenderDirectToPbo (RTRenderer.cs:109-116): max(1, (int)XMath.Round(out * scale)) in float, ties to even."""
        s = np.float32(self.render_scale if render_scale is None else render_scale)
        out_w, out_h = max(1, out_width), max(1, out_height)
        return (max(1, int(np.rint(np.float32(out_w) * s))), max(1, int(np.rint(np.float32(out_h) * s))))

    def advance_sun(self, dt):
        """The sun animation of RenderDirectToPbo (RTRenderer.cs:169-172), all in float: dt clamped by XMath.Clamp = Max(Min(dt, 0.1f), 0f)
        with the host's Min / Max (a NaN dt stays NaN), one wrap by the float 2*pi."""
        with np.errstate(all="ignore"):
            dtc = _host_fmax(_host_fmin(np.float32(dt), np.float32(0.1)), np.float32(0.0))
            az = np.float32(self.sun_azimuth) + np.float32(self.sun_speed) * dtc
            if az >= TWO_PI_F:
                az = az - TWO_PI_F
            elif az < np.float32(0.0):
                az = az + TWO_PI_F
        self.sun_azimuth = np.float32(az)
        return self.sun_azimuth

    def make_params(self, width, height, frame, dt=0.0):
        """Parameter assembly of RenderDirectToPbo (RTRenderer.cs:119-202) at an internal size of width x height."""
        w, h = max(1, width), max(1, height)
        bake_camera_derived(self.camera, w, h)
        bake_camera_derived(self.prev_camera, w, h)
        temporal_seed = 0 if self.rng_lock_noise == 0 else random.randint(-2 ** 31, 2 ** 31 - 2)    # Random.Shared.Next(int.MinValue, int.MaxValue)
        self.advance_sun(dt)
        p = T.FrameParams()
        p.width, p.height, p.frame = w, h, frame
        p.cam = copy_camera(self.camera)
        p.prevCam = copy_camera(self.prev_camera)
        p.dirLightDir = T.f3(*sun_direction(self.sun_azimuth, self.sun_elevation))
        p.dirLightRadiance = T.f3(*self.dir_light_radiance)
        p.skyTintTop = T.f3(*self.sky_tint_top)
        p.skyTintBottom = T.f3(*self.sky_tint_bottom)
        p.debugCamSeq = 0
        p.enableTemporalReuse = self.enable_temporal_reuse
        p.enableSpatialReuse = self.enable_spatial_reuse
        p.rngLockNoise = temporal_seed
        p.spp = self.spp
        p.maxDepth = self.max_depth
        self.last_made_params = p
        return p

    def end_frame(self):
        """_prevCamera = _camera (RTRenderer.cs:236)."""
        self.prev_camera = copy_camera(self.camera)

    def host_frame(self, out_width, out_height, frame, dt=0.0, render_scale=None):
        """Everything RenderDirectToPbo does on the host for one frame, in its order: (FrameParams, inW, inH); the camera hand-off
        of the frame's end included.  RTRenderer.render_direct runs the device work between make_params and end_frame."""
        in_w, in_h = self.internal_size(out_width, out_height, render_scale)
        p = self.make_params(in_w, in_h, frame, dt)
        self.end_frame()
        return p, in_w, in_h


class RTRenderer(FrameHost):
    """Frame orchestration of RTRenderer.RenderDirectToPbo (RTRenderer.cs:105-236) over one hrt_ctx; the host half is FrameHost.
    The PBO map of the presentation step is out of scope (present() returns the display image)."""

    def __init__(self, device_ids=None, width=1280, height=720, build_default_scene=False, library=None):
        L = self._L = library or lib()
        ids = list(device_ids) if device_ids is not None else [0]
        arr = (C.c_int * len(ids))(*ids)
        h = C.c_void_p()
        rc = L.hrt_create(arr, len(ids), C.byref(h))
        if rc != 0:
            raise HrtError(rc, (L.hrt_last_error(None) or b"").decode())
        self._ctx = h
        self.n_devices = len(ids)
        FrameHost.__init__(self, width, height)
        self.scene = None
        self.last_params = None
        self.device_ids = ids
        self.last_query_ms = 0.0              # device time of the last trace_rays (HIP events, max over device slots)
        if build_default_scene:
            s = Scene()
            s.build_default_scene()
            self.commit(s)

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.hrt_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def _check(self, rc):
        if rc != 0:
            raise HrtError(rc, (self._L.hrt_last_error(self._ctx) or b"").decode())

    def commit(self, scene_or_desc):
        """SceneManager.Commit -> BvhManager.BuildOrRefit -> Scene.UploadAll."""
        if isinstance(scene_or_desc, T.SceneDesc):
            d = scene_or_desc
        else:
            self.scene = scene_or_desc
            d = scene_or_desc.desc()
        self._check(self._L.hrt_scene_upload(self._ctx, C.byref(d)))

    def update_instances(self, ids, transforms, policy=T.REBUILD_AUTO):
        """BvhManager.BuildOrRefit(scene, policy) for moved instances, on the device (hrt_scene_update_instances).
        ids: instance ids; transforms: Affine3x4 objects or an (n, 12) float32 array, row-major 3x4.  Returns BvhUpdateStats."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if len(transforms) and isinstance(transforms[0], T.Affine3x4):
            xf = np.array([[getattr(a, f"m{r}{c}") for r in range(3) for c in range(4)] for a in transforms], dtype=np.float32)
        else:
            xf = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 12)
        if xf.shape[0] != ids.size:
            raise ValueError("one transform per instance id")
        st = T.BvhUpdateStats()
        self._check(self._L.hrt_scene_update_instances(self._ctx, ids.ctypes.data if ids.size else None, ids.size,
                                                     xf.ctypes.data if ids.size else None, policy, C.byref(st)))
        return st

    def update_positions(self, first_vertex, positions, policy=T.REBUILD_AUTO):
        """Deforming meshes: meshPositions[first_vertex : first_vertex + n] := positions ((n, 3) float32); every triangle-mesh
        BLAS is refitted on the device, then the TLAS per `policy` (hrt_scene_update_positions).  Returns BvhUpdateStats."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        st = T.BvhUpdateStats()
        self._check(self._L.hrt_scene_update_positions(self._ctx, int(first_vertex), pos.shape[0], pos.ctypes.data if pos.size else None,
                                                     policy, C.byref(st)))
        return st

    def update_spheres(self, first_sphere, spheres, policy=T.REBUILD_AUTO):
        """spheres[first_sphere : first_sphere + n] := spheres (a list of T.Sphere or a structured numpy array); sphere-set BLASes
        are refitted on the device, then the TLAS per `policy` (hrt_scene_update_spheres).  Returns BvhUpdateStats."""
        if isinstance(spheres, np.ndarray):
            buf = np.ascontiguousarray(spheres)
            n, ptr = len(buf), buf.ctypes.data
        else:
            buf = (T.Sphere * max(1, len(spheres)))(*spheres)
            n, ptr = len(spheres), C.addressof(buf)
        st = T.BvhUpdateStats()
        self._check(self._L.hrt_scene_update_spheres(self._ctx, int(first_sphere), n, ptr if n else None, policy, C.byref(st)))
        return st

    def download_array(self, name, slot=0):
        """One of the 15 scene arrays as it is on the device now (numpy structured array / int32)."""
        names = [n for n, _ in T.SCENE_ARRAYS]
        k = names.index(name)
        cnt = C.c_int64()
        self._check(self._L.hrt_scene_download_array(self._ctx, slot, k, None, 0, C.byref(cnt)))
        out = np.zeros(max(1, cnt.value), dtype=T.np_dtype(T.SCENE_ARRAYS[k][1]))
        self._check(self._L.hrt_scene_download_array(self._ctx, slot, k, out.ctypes.data, len(out), C.byref(cnt)))
        return out[:cnt.value]

    def download_tlas(self, slot=0):
        """(tlasNodes, tlasInstanceIndices, instances) of the TLAS in use, as ctypes arrays in the reference's layout."""
        cnt = (C.c_int64 * 3)()
        self._check(self._L.hrt_scene_download_tlas(self._ctx, slot, None, 0, None, 0, None, 0, cnt))
        nodes = (T.BvhNode * max(1, cnt[0]))()
        idx = (C.c_int32 * max(1, cnt[1]))()
        inst = (T.InstanceRecord * max(1, cnt[2]))()
        self._check(self._L.hrt_scene_download_tlas(self._ctx, slot, nodes, cnt[0], idx, cnt[1], inst, cnt[2], cnt))
        return nodes, idx, inst, tuple(cnt)

    def render_params(self, params, outputs=None, flags=0, rows=None, strips=None):
        """The two launches + sync for an explicit FrameParams.  Returns Stats.
        rows=(y0,y1) restricts the frame to a row range, strips=(n,i) to every n-th 8-row strip of it;
        flags & FLAG_NO_SYNC only enqueues (collect with synchronize())."""
        st = T.Stats()
        opts = T.RenderOpts(flags, rows[0] if rows else 0, rows[1] if rows else 0,
                            strips[0] if strips else 1, strips[1] if strips else 0)
        self._check(self._L.hrt_render_frame(self._ctx, C.byref(params), C.byref(opts),
                                           C.byref(outputs) if outputs is not None else None, C.byref(st)))
        self.last_params = params
        return st

    def render_progressive(self, params, sample_begin, outputs=None, flags=0, rows=None, strips=None):
        """Samples [sample_begin, params.spp) of the frame `params` describes (hrt_render_progressive): afterwards every output is
        bit for bit the frame render_params(params) gives.  sample_begin = 0 starts a progressive frame; sample_begin > 0 continues
        the last one, with params equal to its params except spp, sample_begin = its spp, and the same rows, strips and
        REFERENCE_LAYOUT / MEGAKERNEL / STREAMED / TREELETS flags.  FLAG_NO_SYNC only enqueues (outputs must be None).  Returns Stats."""
        sample_begin = _progressive_args(params.spp, sample_begin, flags, outputs)
        st = T.Stats()
        opts = T.RenderOpts(flags, rows[0] if rows else 0, rows[1] if rows else 0,
                            strips[0] if strips else 1, strips[1] if strips else 0)
        self._check(self._L.hrt_render_progressive(self._ctx, C.byref(params), C.byref(opts), sample_begin,
                                                   C.byref(outputs) if outputs is not None else None, C.byref(st)))
        self.last_params = params
        return st

    def refine(self, params, schedule, outputs=None, flags=0):
        """Renders the frame `params` describes progressively, one call per entry of `schedule`: cumulative sample counts such as
        (8, 32, 256).  Returns a generator that yields (spp_so_far, Stats) after each call, when the outputs (and present()) show the frame at
        spp_so_far samples; stop iterating to stop early.  params.spp is ignored; `params` is not modified.
        The schedule and flags are checked here, before the first call."""
        steps = _refine_schedule(schedule)
        _progressive_args(steps[0], 0, flags, outputs)
        p = T.FrameParams.from_buffer_copy(params)

        def run():
            begin = 0
            for spp in steps:
                p.spp = spp
                st = self.render_progressive(p, begin, outputs, flags)
                begin = spp
                yield spp, st
        return run()

    def render_frame(self, width, height, frame, dt=0.0, outputs=None, flags=0, rows=None):
        """RenderDirectToPbo(pbo, width, height, frame, dt) without the presentation step, with width x height as the internal size
        (a render scale of 1); render_direct applies the render scale."""
        p = self.make_params(width, height, frame, dt)
        st = self.render_params(p, outputs, flags, rows)
        self.end_frame()
        return st

    def synchronize(self):
        """Waits for frames enqueued with FLAG_NO_SYNC; Stats.kernel_ms are sums over Stats.frames frames."""
        st = T.Stats()
        self._check(self._L.hrt_synchronize(self._ctx, C.byref(st)))
        return st

    def frame_times(self, launch=1, slot=0):
        """Per-frame HIP-event times (ms) of the frames the last synchronize() / blocking frame collected."""
        n = C.c_int(0)
        self._check(self._L.hrt_frame_times(self._ctx, slot, launch, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), np.float32)
        self._check(self._L.hrt_frame_times(self._ctx, slot, launch, out.ctypes.data, n.value, None))
        return out[:n.value]

    def register_host(self, arrays):
        """Page-locks host arrays used as gather targets (hrt_host_register); arrays: dict or iterable of numpy arrays."""
        for a in (arrays.values() if isinstance(arrays, dict) else arrays):
            self._check(self._L.hrt_host_register(self._ctx, a.ctypes.data, a.nbytes))

    def unregister_host(self, arrays):
        for a in (arrays.values() if isinstance(arrays, dict) else arrays):
            self._check(self._L.hrt_host_unregister(self._ctx, a.ctypes.data))

    def set_workspace_limit(self, max_resident_paths):
        """Caps the streamed pipeline's path workspace (0 = default): larger frames run in sample batches, same results."""
        self._check(self._L.hrt_set_workspace_limit(self._ctx, int(max_resident_paths)))

    def present(self, out_width, out_height, taau=True, out=None, feedback=0.0, sharpness=0.0, clamp_k=0.0, reproject=False, denoised=False):
        """Presentation step of RenderDirectToPbo (RTRenderer.cs:208-231): TAAU resolve, or blit / bilinear upsample.
        reproject (with taau): the history is read where the camera's motion since the last resolved frame puts it
        (HRT_PRESENT_TAAU_REPROJECT, include/hip_raytrace.h).  denoised: resolve the denoised colour of the last denoise() instead of
        the frame's (HRT_PRESENT_DENOISED; an HrtError if the frame is newer than it).  Returns the display-size packed colour as an
        int32 array."""
        if reproject and not taau:
            raise ValueError("reproject is a mode of the TAAU resolve (taau=True)")
        mode = T.PRESENT_TAAU_REPROJECT if reproject else (T.PRESENT_TAAU if taau else T.PRESENT_RESAMPLE)
        if denoised:
            mode |= T.PRESENT_DENOISED
        pp = T.PresentParams(out_width, out_height, mode, feedback, sharpness, clamp_k)
        if out is None:
            out = np.zeros(out_width * out_height, np.int32)
        self._check(self._L.hrt_present(self._ctx, C.byref(pp), out.ctypes.data))
        return out

    def present_ms(self):
        """HIP-event time of the kernel of the last present() (hrt_present_time)."""
        ms = C.c_float(0.0)
        self._check(self._L.hrt_present_time(self._ctx, C.byref(ms)))
        return ms.value

    def render_direct(self, out_width, out_height, frame, dt=0.0, render_scale=None, taau=None, flags=0, outputs=None, reproject=None):
        """RenderDirectToPbo(pbo, width, height, frame, dt) end to end: internal size = round(out * renderScale) (RTRenderer.cs:109-116;
        render_scale / taau default to the fields render_scale = 0.67f / enable_taau), the two launches, then the presentation step.
        outputs (optional, internal size) also receives the internal arrays.  reproject (default: the field enable_reproject = False)
        selects the reprojecting TAAU when TAAU is on.  Returns (display colour, Stats)."""
        out_w, out_h = max(1, out_width), max(1, out_height)
        in_w, in_h = self.internal_size(out_w, out_h, render_scale)
        p = self.make_params(in_w, in_h, frame, dt)
        st = self.render_params(p, outputs, flags)
        taau = self.enable_taau if taau is None else taau
        out = self.present(out_w, out_h, taau, reproject=bool(taau and (self.enable_reproject if reproject is None else reproject)))
        self.end_frame()
        return out, st

    def motion_vectors(self, from_cam=None, slot=None):
        """Camera motion vectors of the last full-image frame (hrt_motion_vectors): for internal pixel i, where its surface point was
        in the image of from_cam (a T.Camera; default: the frame's prevCam) minus where it is now, in pixels; NaN where the point is
        behind either camera.  slot=None: host path over every device slot, returns an (height, width, 2) float32 numpy array.
        slot=0: device path, returns a torch tensor of that shape on slot 0's device, no host copy."""
        v = self.device_views(0)
        w, h = v.width, v.height
        cam = None if from_cam is None else C.byref(from_cam)
        ms = C.c_float(0.0)
        if slot is None:
            out = np.zeros((h, w, 2), np.float32)
            self._check(self._L.hrt_motion_vectors(self._ctx, cam, out.ctypes.data, -1, C.byref(ms)))
        else:
            if slot != 0:
                raise ValueError("motion vectors stay on the device of slot 0 only (slot=0), or come to the host (slot=None)")
            import torch                                       # lazy: the host path needs no torch
            out = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda:%d" % self.device_ids[0])
            torch.cuda.synchronize(out.device)                 # the library works on its own streams
            self._check(self._L.hrt_motion_vectors(self._ctx, cam, out.data_ptr(), 0, C.byref(ms)))
        self.last_query_ms = ms.value
        return out

    def denoise(self, iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_plane=0.0, demodulate=True, slot=None):
        """Edge-avoiding a-trous filter over the radiance of the last full-image frame, guided by its G-buffer (hrt_denoise,
        include/hip_raytrace.h).  iterations 1..8 (0: 5), iteration i with tap step 1 << i; sigmas <= 0 select 4.0 / 0.5 / 0.02;
        demodulate=False filters the radiance itself instead of radiance / albedo.  The frame is left as it is; present(...,
        denoised=True) shows the result.  slot=None: returns (radiance (h, w, 3) float32, color (h, w) int32) as numpy arrays.
        slot=0: torch tensors of those shapes over the library's own device planes, no copy: valid until a denoise() at another
        frame size or close(), overwritten by the next denoise()."""
        v = self.device_views(0)
        w, h = v.width, v.height
        dp = T.DenoiseParams(int(iterations), 0 if demodulate else T.DENOISE_NO_DEMODULATE, sigma_color, sigma_normal, sigma_plane)
        ms = C.c_float(0.0)
        if slot is None:
            rad, col = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.int32)
            self._check(self._L.hrt_denoise(self._ctx, C.byref(dp), rad.ctypes.data, col.ctypes.data, C.byref(ms)))
            self.last_query_ms = ms.value
            return rad, col
        if slot != 0:
            raise ValueError("the denoised planes live on the device of slot 0 only (slot=0), or come to the host (slot=None)")
        import torch                                       # lazy: the host path needs no torch
        self._check(self._L.hrt_denoise(self._ctx, C.byref(dp), None, None, C.byref(ms)))
        self.last_query_ms = ms.value
        pr, pc = C.c_void_p(), C.c_void_p()
        self._check(self._L.hrt_denoised_buffers(self._ctx, C.byref(pr), C.byref(pc)))
        dev = "cuda:%d" % self.device_ids[0]
        return (_device_plane(torch, pr.value, (h, w, 3), "<f4", dev, self), _device_plane(torch, pc.value, (h, w), "<i4", dev, self))

    def denoise_temporal(self, iterations=0, alpha_color=0.0, alpha_moments=0.0, sigma_lum=0.0, sigma_normal=0.0, sigma_plane=0.0,
                         normal_cos_min=0.0, plane_tol=0.0, max_history=0, demodulate=True, spatial=True, reset=False, slot=None):
        """The temporal denoiser (hrt_denoise_temporal, include/hip_raytrace.h): accumulates the demodulated radiance and its luminance
        moments of the last full-image frame into a reprojected history, then runs a-trous passes whose colour term follows the
        per-pixel variance.  One call per frame; arguments of 0 select the defaults.  spatial=False: plain temporal accumulation;
        reset=True: start from an empty history.  Returns what denoise() returns, in the same planes: present(..., denoised=True) shows
        whichever of the two ran last on the frame."""
        v = self.device_views(0)
        w, h = v.width, v.height
        flags = (0 if demodulate else T.DENOISE_T_NO_DEMODULATE) | (0 if spatial else T.DENOISE_T_NO_SPATIAL) | (T.DENOISE_T_RESET if reset else 0)
        tp = T.DenoiseTemporalParams(int(iterations), flags, alpha_color, alpha_moments, sigma_lum, sigma_normal, sigma_plane,
                                     normal_cos_min, plane_tol, int(max_history))
        ms = C.c_float(0.0)
        if slot is None:
            rad, col = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.int32)
            self._check(self._L.hrt_denoise_temporal(self._ctx, C.byref(tp), rad.ctypes.data, col.ctypes.data, C.byref(ms)))
            self.last_query_ms = ms.value
            return rad, col
        if slot != 0:
            raise ValueError("the denoised planes live on the device of slot 0 only (slot=0), or come to the host (slot=None)")
        import torch                                       # lazy: the host path needs no torch
        self._check(self._L.hrt_denoise_temporal(self._ctx, C.byref(tp), None, None, C.byref(ms)))
        self.last_query_ms = ms.value
        pr, pc = C.c_void_p(), C.c_void_p()
        self._check(self._L.hrt_denoised_buffers(self._ctx, C.byref(pr), C.byref(pc)))
        dev = "cuda:%d" % self.device_ids[0]
        return (_device_plane(torch, pr.value, (h, w, 3), "<f4", dev, self), _device_plane(torch, pc.value, (h, w), "<i4", dev, self))

    def denoise_history(self):
        """The temporal denoiser's current history, copied to the host (hrt_denoise_history_read): dict of color (h, w, 3), variance,
        length (h, w) and moments (h, w, 2) float32 arrays, or None while the history is empty."""
        hv = T.DenoiseHistoryViews()
        self._check(self._L.hrt_denoise_history(self._ctx, C.byref(hv)))
        if not hv.color:
            return None
        n = hv.width * hv.height
        col, mom = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        self._check(self._L.hrt_denoise_history_read(self._ctx, col.ctypes.data, mom.ctypes.data))
        shape = (hv.height, hv.width)
        return dict(color=col[:, :3].reshape(shape + (3,)).copy(), variance=col[:, 3].reshape(shape).copy(),
                    moments=mom[:, :2].reshape(shape + (2,)).copy(), length=mom[:, 2].reshape(shape).copy())

    def reset_history(self):
        self._check(self._L.hrt_reset_history(self._ctx))

    def device_views(self, slot=0):
        v = T.DeviceViews()
        self._check(self._L.hrt_device_buffers(self._ctx, slot, C.byref(v)))
        return v

    def trace_rays(self, origins, dirs, tmax=None, query="closest", slot=None):
        """SceneDeviceViews.TraceClosest / ShadowOcclusion (SceneDeviceViews.cs:30-121) on the scene now on the device, one result per ray
        (hrt_trace_rays).  origins, dirs: (n, 3) float32; dirs are used as given (t is in units of |dir|).  tmax: ShadowOcclusion's
        tMaxWorld, a float or (n,) float32 (default +inf); closest-hit queries have none (TraceClosest starts at 1e30).
        numpy inputs: host path over every device slot; returns a structured array of T.RayHit ("closest") or int32 0/1 ("occluded").
        torch tensors on a GPU: device path on the slot of their device (`slot` picks one of several); returns torch tensors, no host copy:
        "closest" -> dict t, normal, albedo, ior (float32), objId, shade, instance, prim (int32); "occluded" -> int32 (n,).
        A process that hands torch tensors over imports torch before this library is loaded: torch's HIP runtime is then the process's."""
        q = _QUERIES.get(query)
        if q is None:
            raise ValueError("query must be one of %s, not %r" % (sorted(_QUERIES), query))
        if _torch_inputs(origins, dirs):
            return self._trace_rays_torch(q, origins, dirs, tmax, slot)
        o, d = _host_rays(origins, dirs, slot)
        n = o.shape[0]
        rays = _pack_host_rays(o, d, tmax)
        out = np.zeros(n, T.np_dtype(T.RayHit)) if q == T.QUERY_CLOSEST else np.zeros(n, np.int32)
        ms = C.c_float(0.0)
        self._check(self._L.hrt_trace_rays(self._ctx, q, rays.ctypes.data if n else None, n, out.ctypes.data if n else None, -1, C.byref(ms)))
        self.last_query_ms = ms.value
        return out

    def _torch_slot(self, device, slot):
        """The device slot of this renderer that torch device `device` is (`slot` picks one of several on it)."""
        import torch
        dev = device.index if device.index is not None else torch.cuda.current_device()
        slots = [i for i, d in enumerate(self.device_ids) if d == dev]
        if slot is None:
            if not slots:
                raise ValueError("no device slot of this renderer is on cuda:%d (slots: %s)" % (dev, self.device_ids))
            return slots[0]
        if slot not in slots:
            raise ValueError("device slot %r is not on cuda:%d (slots: %s)" % (slot, dev, self.device_ids))
        return slot

    def _trace_rays_torch(self, q, origins, dirs, tmax, slot):
        import torch                                       # lazy: the host path needs no torch
        n, tm = _check_torch_rays(origins, dirs, tmax)
        slot = self._torch_slot(origins.device, slot)
        rays = _pack_torch_rays(origins, dirs, tm)
        out = torch.zeros((n, 12) if q == T.QUERY_CLOSEST else (n,), dtype=torch.float32 if q == T.QUERY_CLOSEST else torch.int32,
                          device=origins.device)
        torch.cuda.synchronize(origins.device)               # the library works on its own streams
        ms = C.c_float(0.0)
        self._check(self._L.hrt_trace_rays(self._ctx, q, rays.data_ptr() if n else None, n, out.data_ptr() if n else None, slot, C.byref(ms)))
        self.last_query_ms = ms.value
        return _hit_dict(out) if q == T.QUERY_CLOSEST else out

    def trace_hits(self, origins, dirs, k, tmax=None, totals=False, slot=None):
        """The k nearest accepted hits along each ray (hrt_trace_hits): ShadowOcclusion's walk (SceneDeviceViews.cs:89-121) run to the
        end with TraceClosest's acceptance and records (:30-86, :124-237), ordered by (t, instance, prim).  origins, dirs: (n, 3) float32,
        dirs used as given.  k: 1..T.HITS_MAX.  tmax: a float or (n,) float32 (default +inf).  totals: also return every accepted test.
        numpy inputs: host path over every device slot; returns (hits, counts, totals or None), hits an (n, k) structured array of
        T.RayHit (slots j >= counts[i] hold CLOSEST's miss record).
        torch tensors on a GPU: device path on the slot of their device; returns a dict of tensors t, normal, albedo, ior (float32),
        objId, shade, instance, prim (int32), each (n, k, ...), plus counts (n,) and totals ((n,) or None)."""
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
            raise TypeError("k must be an int, not %r" % (k,))
        k = int(k)
        if not 1 <= k <= T.HITS_MAX:
            raise ValueError("k must be in [1, %d], got %d" % (T.HITS_MAX, k))
        totals = bool(totals)
        if _torch_inputs(origins, dirs):
            return self._trace_hits_torch(origins, dirs, k, tmax, totals, slot)
        o, d = _host_rays(origins, dirs, slot)
        n = o.shape[0]
        rays = _pack_host_rays(o, d, tmax)
        hits = np.zeros((n, k), T.np_dtype(T.RayHit))
        counts = np.zeros(n, np.int32)
        tot = np.zeros(n, np.int32) if totals else None
        ms = C.c_float(0.0)
        self._check(self._L.hrt_trace_hits(self._ctx, rays.ctypes.data if n else None, n, k, hits.ctypes.data if n else None,
                                           counts.ctypes.data if n else None, tot.ctypes.data if (n and totals) else None, -1, C.byref(ms)))
        self.last_query_ms = ms.value
        return hits, counts, tot

    def _trace_hits_torch(self, origins, dirs, k, tmax, totals, slot):
        import torch
        n, tm = _check_torch_rays(origins, dirs, tmax)
        slot = self._torch_slot(origins.device, slot)
        rays = _pack_torch_rays(origins, dirs, tm)
        out = torch.zeros((n, k, 12), dtype=torch.float32, device=origins.device)
        counts = torch.zeros(n, dtype=torch.int32, device=origins.device)
        tot = torch.zeros(n, dtype=torch.int32, device=origins.device) if totals else None
        torch.cuda.synchronize(origins.device)               # the library works on its own streams
        ms = C.c_float(0.0)
        self._check(self._L.hrt_trace_hits(self._ctx, rays.data_ptr() if n else None, n, k, out.data_ptr() if n else None,
                                           counts.data_ptr() if n else None, tot.data_ptr() if (n and totals) else None, slot, C.byref(ms)))
        self.last_query_ms = ms.value
        return dict(_hit_dict(out), counts=counts, totals=tot)

    def trace_paths(self, origins, dirs, params, first_key=0, flags=0, slot=None):
        """PathTraceKernel (RTRay.cs:203-325) along caller rays (hrt_trace_paths): ray i is shaded as pixel key j = first_key + i of
        the frame `params` describes (RNG pixel (j % width, j // width)), with reuse off, its primary vertex TraceClosest(ray) and
        the ray's own origin / direction where the frame uses the camera's (view direction, miss sky, depth).  origins, dirs: (n, 3)
        float32, dirs used as given.  Camera rays (camera_rays(params)) give the frame's radiance, color, depth and objectId bit for bit.
        numpy inputs: host path over every device slot; returns a structured array of T.PathResult.
        torch tensors on a GPU: device path on the slot of their device; returns a dict of tensors radiance (n, 3) float32,
        color, objId int32, depth float32."""
        if not isinstance(params, T.FrameParams):
            raise TypeError("params must be a FrameParams")
        if params.enableTemporalReuse or params.enableSpatialReuse:
            raise ValueError("trace_paths runs with ReSTIR reuse off: set enableTemporalReuse and enableSpatialReuse to 0")
        if params.width <= 0 or params.maxDepth < 0:
            raise ValueError("params.width must be positive and params.maxDepth >= 0")
        flags = int(flags)
        if flags & ~T.PATH_FLAGS:
            raise ValueError("trace_paths takes only FLAG_REFERENCE_LAYOUT, FLAG_MEGAKERNEL, FLAG_STREAMED and FLAG_TREELETS, not %#x" % flags)
        first_key = int(first_key)
        if first_key < 0:
            raise ValueError("first_key must be >= 0")
        if _torch_inputs(origins, dirs):
            return self._trace_paths_torch(origins, dirs, params, first_key, flags, slot)
        o, d = _host_rays(origins, dirs, slot)
        n = o.shape[0]
        if first_key + n > 0x7FFFFFFF:
            raise ValueError("first_key + n exceeds 2^31 - 1")
        rays = _pack_host_rays(o, d, _NO_TMAX)
        out = np.zeros(n, T.np_dtype(T.PathResult))
        ms = C.c_float(0.0)
        self._check(self._L.hrt_trace_paths(self._ctx, C.byref(params), flags, rays.ctypes.data if n else None, n, first_key,
                                            out.ctypes.data if n else None, -1, C.byref(ms)))
        self.last_query_ms = ms.value
        return out

    def _trace_paths_torch(self, origins, dirs, params, first_key, flags, slot):
        import torch                                       # lazy: the host path needs no torch
        n, _ = _check_torch_rays(origins, dirs, _NO_TMAX)
        if first_key + n > 0x7FFFFFFF:
            raise ValueError("first_key + n exceeds 2^31 - 1")
        slot = self._torch_slot(origins.device, slot)
        rays = _pack_torch_rays(origins, dirs, _NO_TMAX)
        out = torch.zeros((n, 8), dtype=torch.float32, device=origins.device)
        torch.cuda.synchronize(origins.device)               # the library works on its own streams
        ms = C.c_float(0.0)
        self._check(self._L.hrt_trace_paths(self._ctx, C.byref(params), flags, rays.data_ptr() if n else None, n, first_key,
                                            out.data_ptr() if n else None, slot, C.byref(ms)))
        self.last_query_ms = ms.value
        ints = out.view(torch.int32)
        return dict(radiance=out[:, 0:3], color=ints[:, 3], depth=out[:, 4], objId=ints[:, 5])

    @staticmethod
    def camera_rays(params):
        """The primary rays of the frame `params` describes (RTRay.cs:120-126, Ray.GenerateRay RTUtils.cs:13-17), in pixel order:
        (origins, dirs) as (width*height, 3) float32, with pick's operation order, vectorised."""
        cam = params.cam
        f = np.float32
        v3 = lambda a: np.array([a.X, a.Y, a.Z], np.float32)
        w, h = int(params.width), int(params.height)
        idx = np.arange(w * h, dtype=np.int64)
        u = ((idx % max(1, w)).astype(np.float32) + f(0.5)) / f(max(1, w))
        v = ((idx // max(1, w)).astype(np.float32) + f(0.5)) / f(max(1, h))
        ll, hz, vt, org = v3(cam.lowerLeft), v3(cam.horizontal), v3(cam.vertical), v3(cam.origin)
        d = ((ll[None, :] + hz[None, :] * u[:, None]) + vt[None, :] * v[:, None]) - org[None, :]
        inv = f(1.0) / np.sqrt(np.maximum(f(1e-20), (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))   # Normalize, Float3.cs:91-95
        d = (d * inv[:, None]).astype(np.float32)
        return np.broadcast_to(org, d.shape).astype(np.float32), d

    def pick(self, width, height, x, y):
        """The closest hit under pixel (x, y) of a width x height image (row 0 = bottom row): the pixel-centre primary ray of the
        primary-visibility launch (RTRay.cs:120-126, Ray.GenerateRay RTUtils.cs:13-17) from the camera of the last make_params,
        traced with trace_rays.  Returns one T.RayHit record (numpy)."""
        if self.last_made_params is None:
            raise RuntimeError("pick needs the camera of a frame: call make_params / render_frame first")
        cam = self.last_made_params.cam
        f = np.float32
        v3 = lambda a: (f(a.X), f(a.Y), f(a.Z))
        u = (f(x) + f(0.5)) / f(max(1, width))
        v = (f(y) + f(0.5)) / f(max(1, height))
        ll, hz, vt, org = v3(cam.lowerLeft), v3(cam.horizontal), v3(cam.vertical), v3(cam.origin)
        d = [((ll[k] + hz[k] * u) + vt[k] * v) - org[k] for k in range(3)]
        inv = f(1.0) / np.sqrt(max(f(1e-20), (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))        # Normalize, Float3.cs:91-95
        o = np.array([org], np.float32)
        dd = np.array([[d[0] * inv, d[1] * inv, d[2] * inv]], np.float32)
        return self.trace_rays(o, dd)[0]

    def math_exhaustive(self, which):
        """(mismatches, bits of the first one) of a trimmed device function against its IEEE definition over its whole domain."""
        n, first = C.c_uint64(0), C.c_uint32(0)
        self._check(self._L.hrt_math_exhaustive(self._ctx, which, C.byref(n), C.byref(first)))
        return n.value, first.value

    def math_probe(self, fn, x, y=None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        yy = np.ascontiguousarray(y, dtype=np.float32) if y is not None else None
        self._check(self._L.hrt_math_probe(self._ctx, fn, x.size, x.ctypes.data, yy.ctypes.data if yy is not None else None, out.ctypes.data))
        return out


# ------------------------------------------------------------------ SceneManager / BvhManager (Engine/SceneManager.cs, BvhManager.cs)
_QUERIES = {"closest": T.QUERY_CLOSEST, "occluded": T.QUERY_OCCLUDED}


_PROGRESSIVE_FORBIDDEN = {T.FLAG_COUNTERS: "FLAG_COUNTERS", T.FLAG_PRIMARY_ONLY: "FLAG_PRIMARY_ONLY",
                          T.FLAG_SKIP_PRIMARY: "FLAG_SKIP_PRIMARY", T.FLAG_EXCHANGED: "FLAG_EXCHANGED"}


class _DevicePlane:
    """A device plane of the library through __cuda_array_interface__; keeps its renderer alive."""

    def __init__(self, ptr, shape, typestr, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


def _device_plane(torch, ptr, shape, typestr, device, owner):
    return torch.as_tensor(_DevicePlane(ptr, shape, typestr, owner), device=device)


def _progressive_args(spp, sample_begin, flags, outputs):
    """The argument rules of hrt_render_progressive, checked before the library is called.  Returns sample_begin as an int."""
    if isinstance(sample_begin, bool) or not isinstance(sample_begin, (int, np.integer)):
        raise TypeError("sample_begin must be an int, got %s" % type(sample_begin).__name__)
    sample_begin = int(sample_begin)
    if sample_begin < 0:
        raise ValueError("sample_begin must be >= 0, got %d" % sample_begin)
    if spp < 1:
        raise ValueError("params.spp must be >= 1, got %d" % spp)
    if spp <= sample_begin:
        raise ValueError("params.spp (%d) must exceed sample_begin (%d)" % (spp, sample_begin))
    for bit, name in _PROGRESSIVE_FORBIDDEN.items():
        if flags & bit:
            raise ValueError("%s cannot be used with progressive frames" % name)
    if (flags & T.FLAG_NO_SYNC) and outputs is not None:
        raise ValueError("FLAG_NO_SYNC calls cannot gather to host: outputs must be None")
    return sample_begin


def _refine_schedule(schedule):
    steps = [int(s) for s in schedule]
    if not steps:
        raise ValueError("schedule must name at least one cumulative sample count")
    if steps[0] < 1:
        raise ValueError("schedule must start at >= 1 samples, got %d" % steps[0])
    for a, b in zip(steps, steps[1:]):
        if b <= a:
            raise ValueError("schedule must be strictly increasing cumulative sample counts, got %d after %d" % (b, a))
    return steps


def _rays_arg(a, name):
    if not isinstance(a, np.ndarray):
        raise TypeError("%s must be a numpy array or a torch tensor, got %s" % (name, type(a).__name__))
    if a.dtype != np.float32:
        raise ValueError("%s must be float32, got %s" % (name, a.dtype))
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s must have shape (n, 3), got %s" % (name, a.shape))
    return a


def _tmax_arg(tmax, n):
    if tmax is None:
        return np.float32(np.inf)
    if np.isscalar(tmax):
        return np.float32(tmax)
    t = np.asarray(tmax)
    if t.dtype != np.float32 or t.shape != (n,):
        raise ValueError("tmax must be a float or an (n,) float32 array, got %s %s" % (t.dtype, t.shape))
    return t


# what trace_rays / trace_hits / trace_paths and their torch twins share
_NO_TMAX = object()            # trace_paths: its rays carry no tmax, the column stays 0


def _torch_inputs(origins, dirs):
    """True: both are torch tensors (device path); False: neither is (host path).  A mix is refused."""
    is_torch = [type(a).__module__.split(".")[0] == "torch" for a in (origins, dirs)]
    if any(is_torch) and not all(is_torch):
        raise TypeError("origins and dirs must both be numpy arrays or both torch tensors")
    return all(is_torch)


def _host_rays(origins, dirs, slot):
    o, d = _rays_arg(origins, "origins"), _rays_arg(dirs, "dirs")
    if o.shape != d.shape:
        raise ValueError("origins and dirs differ in shape: %s vs %s" % (o.shape, d.shape))
    if slot is not None:
        raise ValueError("slot selects the device of torch inputs; host arrays are split over every device slot")
    return o, d


def _pack_host_rays(o, d, tmax):
    """(n, 8) float32: hrt_ray's origin, tmax, direction, pad."""
    n = o.shape[0]
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    if tmax is not _NO_TMAX:
        rays[:, 3] = _tmax_arg(tmax, n)
    return rays


def _check_torch_rays(origins, dirs, tmax):
    """Returns n and what goes into the tmax column (a float or an (n,) tensor on the rays' device)."""
    import torch                                       # lazy: the host path needs no torch
    for name, a in (("origins", origins), ("dirs", dirs)):
        if a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != 3:
            raise ValueError("%s must be an (n, 3) float32 tensor, got %s %s" % (name, tuple(a.shape), a.dtype))
        if a.device.type != "cuda":
            raise ValueError("%s: torch inputs must live on a GPU (numpy arrays take the host path)" % name)
    if origins.shape != dirs.shape:
        raise ValueError("origins and dirs differ in shape: %s vs %s" % (tuple(origins.shape), tuple(dirs.shape)))
    if origins.device != dirs.device:
        raise ValueError("origins and dirs live on different devices")
    n = origins.shape[0]
    if tmax is _NO_TMAX:
        return n, tmax
    if tmax is None or isinstance(tmax, (int, float, np.floating)):
        return n, float("inf") if tmax is None else float(np.float32(tmax))
    tm = torch.as_tensor(tmax, device=origins.device)
    if tm.dtype != torch.float32 or tuple(tm.shape) != (n,):
        raise ValueError("tmax must be a float or an (n,) float32 array")
    return n, tm


def _pack_torch_rays(origins, dirs, tm):
    import torch
    rays = torch.zeros((origins.shape[0], 8), dtype=torch.float32, device=origins.device)
    rays[:, 0:3], rays[:, 4:7] = origins, dirs
    if tm is not _NO_TMAX:
        rays[:, 3] = tm
    return rays


def _hit_dict(out):
    """The fields of T.RayHit as views of a (..., 12) float32 tensor of records."""
    import torch
    ints = out[..., 8:12].view(torch.int32)
    return dict(t=out[..., 0], normal=out[..., 1:4], albedo=out[..., 4:7], ior=out[..., 7],
                objId=ints[..., 0], shade=ints[..., 1], instance=ints[..., 2], prim=ints[..., 3])


class SceneManager:
    """SceneManager (SceneManager.cs:12-38) over one RTRenderer: Scene, BuildDefaultScene, LoadObjInstance, Commit(policy),
    ReplaceScene.  Commit is BvhManager.BuildOrRefit (BvhManager.cs:27) with the RebuildPolicy honoured: the first commit, and
    any commit after the scene's structure changed (instances, spheres, meshes added), uploads everything as the reference
    does; a commit after only instance transforms moved (set_instance_transform) updates the device copy in place."""

    def __init__(self, renderer, existing_scene=None):
        if renderer is None:
            raise ValueError("renderer is None")                    # ArgumentNullException(nameof(cuda))
        self._r = renderer
        self._scene = existing_scene if existing_scene is not None else Scene()
        self._uploaded_shape = None
        self._moved = {}
        self.last_update = None

    @property
    def scene(self):
        return self._scene

    def build_default_scene(self):
        self._scene.build_default_scene()

    def load_obj_instance(self, obj_path, object_to_world=None, uniform_scale=1.0):
        return self._scene.load_obj_instance(obj_path, object_to_world, uniform_scale)

    def set_instance_transform(self, inst_id, object_to_world):
        """Moves an instance of the scene; takes effect at the next commit."""
        self._scene.set_instance_transform(inst_id, object_to_world)
        self._moved[int(inst_id)] = object_to_world

    def _shape(self):
        d = self._scene.desc()
        return tuple(getattr(d, "n_" + n) for n, _ in T.SCENE_ARRAYS)

    def commit(self, policy=T.REBUILD_AUTO):
        shape = self._shape()
        if self._uploaded_shape != shape:
            self._scene.rebuild_tlas()                                # a host that added or moved things before its first commit
            self._r.commit(self._scene)
            self._uploaded_shape = self._shape()
            self.last_update = None
        elif self._moved:
            ids = sorted(self._moved)
            self.last_update = self._r.update_instances(ids, [self._moved[i] for i in ids], policy)
        self._moved = {}

    def replace_scene(self, new_scene, rebuild_immediately=True, policy=T.REBUILD_AUTO):
        if new_scene is None:
            raise ValueError("new_scene is None")
        self._scene = new_scene
        self._uploaded_shape = None
        self._moved = {}
        if rebuild_immediately:
            self.commit(policy)


def device_count():
    return lib().hrt_device_count()
