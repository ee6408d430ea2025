"""Host-side objects over the C ABI: Mesh, BspTree, Bvh (the Rust structures
that feed the GPU, src/mesh.rs and src/data_structures/) and Context (the
HIP device/stream handle that replaces src/gpu_handles.rs plus the GPU
binding layer src/bindings/)."""
import ctypes as C

import numpy as np

from . import _ffi as F


def _vp(ptr):
    """A device or host address as a ctypes argument; 0 and None are the null pointer."""
    return C.c_void_p(ptr) if ptr else None


def _mats_from(ptr, n):
    if n == 0:
        return np.zeros((0, 16), dtype=np.float32)
    raw = np.ctypeslib.as_array(C.cast(ptr, F.f32p), shape=(n * 16,)).copy()
    return raw.reshape(n, 16)


class Mesh:
    """Mesh (src/mesh.rs:35-41): vertices/normals float4, indices (v0,v1,v2,material)."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle) if not isinstance(handle, C.c_void_p) else handle

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and F._lib is not None:
            F._lib.rt_mesh_free(self._h)
            self._h = C.c_void_p(None)

    @property
    def handle(self):
        return self._h

    # -- constructors -----------------------------------------------------
    @classmethod
    def from_obj(cls, path):
        """Mesh::from_obj (src/mesh.rs:78-92)."""
        h = C.c_void_p()
        F.check(F.lib().rt_mesh_load_obj(str(path).encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, vertices, indices, normals=None, materials=None):
        pos = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 4)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 4)
        nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 4)
        mats = None if materials is None else np.ascontiguousarray(materials, dtype=np.float32).reshape(-1, 16)
        h = C.c_void_p()
        F.check(F.lib().rt_mesh_from_arrays(F.as_f32p(pos), None if nrm is None else F.as_f32p(nrm), pos.shape[0],
                                            F.as_u32p(idx), idx.shape[0],
                                            None if mats is None else C.cast(mats.ctypes.data, C.POINTER(F.Material)),
                                            0 if mats is None else mats.shape[0], C.byref(h)))
        return cls(h)

    @classmethod
    def synth_bunny(cls, ntris=69451, seed=0x0B0B):
        h = C.c_void_p()
        F.check(F.lib().rt_mesh_synth_bunny(ntris, seed, C.byref(h)))
        return cls(h)

    @classmethod
    def synth_soup(cls, ntris, seed=0x5EED):
        h = C.c_void_p()
        F.check(F.lib().rt_mesh_synth_soup(ntris, seed, C.byref(h)))
        return cls(h)

    @classmethod
    def grid(cls, src, nx, nz, spacing):
        h = C.c_void_p()
        F.check(F.lib().rt_mesh_synth_grid(src.handle, nx, nz, spacing, C.byref(h)))
        return cls(h)

    def scale(self, factor):
        """Mesh::scale (src/mesh.rs:246-252)."""
        F.check(F.lib().rt_mesh_scale(self._h, factor))
        return self

    # -- views --------------------------------------------------------------
    def _view(self):
        v = F.MeshView()
        F.check(F.lib().rt_mesh_view_get(self._h, C.byref(v)))
        return v

    @property
    def ntris(self):
        return int(self._view().ntris)

    def arrays(self):
        """Copies: (vertices[n,4], normals[n,4], indices[t,4], materials[m,16], lights[l])."""
        v = self._view()
        return (F.np_from(v.vertices, v.nverts, np.float32, 4), F.np_from(v.normals, v.nverts, np.float32, 4),
                F.np_from(v.indices, v.ntris, np.uint32, 4), _mats_from(v.materials, v.nmats),
                F.np_from(v.lights, v.nlights, np.uint32))

    # -- acceleration structures (src/mesh.rs:229-239) -------------------
    def bsp_tree(self, max_depth=20, max_leaf=4, nthreads=0):
        return BspTree.build(self, max_depth, max_leaf, nthreads)

    def bvh(self, max_prims=4):
        return Bvh.build(self, max_prims)


class BspTree:
    """BspTree + BspTreeIntermediate (src/data_structures/bsp_tree.rs:45-347)."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and F._lib is not None:
            F._lib.rt_bsp_free(self._h)
            self._h = C.c_void_p(None)

    @classmethod
    def build(cls, mesh, max_depth=20, max_leaf=4, nthreads=0):
        h = C.c_void_p()
        F.check(F.lib().rt_bsp_build(mesh.handle, max_depth, max_leaf, nthreads, C.byref(h)))
        return cls(h)

    @property
    def handle(self):
        return self._h

    def arrays(self):
        """(bsp_tree[n,4] u32, bsp_planes[n] f32, tree_ids[k] u32, aabb[8] f32, max_depth)."""
        v = F.BspView()
        F.check(F.lib().rt_bsp_view_get(self._h, C.byref(v)))
        return (F.np_from(v.tree, v.nnodes, np.uint32, 4), F.np_from(v.planes, v.nnodes, np.float32),
                F.np_from(v.ids, v.nids, np.uint32), np.array(list(v.aabb), dtype=np.float32), int(v.max_depth))


class Bvh:
    """hlbvh::Bvh flattened (src/data_structures/hlbvh.rs:195-239)."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and F._lib is not None:
            F._lib.rt_bvh_free(self._h)
            self._h = C.c_void_p(None)

    @classmethod
    def build(cls, mesh, max_prims=4):
        h = C.c_void_p()
        F.check(F.lib().rt_bvh_build(mesh.handle, max_prims, C.byref(h)))
        return cls(h)

    @property
    def handle(self):
        return self._h

    def arrays(self):
        """(nodes[n,8] u32 view of GpuNode, tri_ids[k] u32)."""
        v = F.BvhView()
        F.check(F.lib().rt_bvh_view_get(self._h, C.byref(v)))
        raw = F.np_from(C.cast(v.nodes, F.u32p), v.nnodes, np.uint32, 8)
        return raw, F.np_from(v.tri_ids, v.nids, np.uint32)


def make_uniform(eye, target, up, constant, width, height, selection1=0, subdiv=1, aspect=None, iteration=0,
                 selection2=0, use_texture=0, uv_scale=(1.0, 1.0)):
    """Uniform (src/bindings/uniform.rs:6-34) for a headless W x H frame; selection2,
    use_texture and uv_scale default to the reference's (uniform.rs:152-156)."""
    u = F.Uniform()
    u.camera_pos[:] = [float(v) for v in eye]
    u.camera_look_at[:] = [float(v) for v in target]
    u.camera_up[:] = [float(v) for v in up]
    u.camera_constant = float(constant)
    u.aspect_ratio = float(np.float32(width) / np.float32(height)) if aspect is None else float(aspect)
    u.selection1 = selection1
    u.selection2 = selection2
    u.subdivision_level = subdiv
    u.use_texture = use_texture
    u.iteration = iteration
    u.uv_scale[:] = [float(v) for v in uv_scale]
    u.resolution[:] = [width, height]
    return u


# include/rt.h rt_ray_hit
RAY_HIT_DTYPE = np.dtype([("tri", "<u4"), ("dist", "<f4"), ("beta", "<f4"), ("gamma", "<f4"), ("ntested", "<u4"),
                          ("tested_fnv", "<u4"), ("tmin", "<f4"), ("tmax", "<f4")])


class DeviceBuffer:
    """HBM allocation owned by a Context (frame buffers)."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        F.check(F.lib().rt_device_alloc(ctx.handle, self.nbytes, C.byref(p)), ctx.handle)
        self.ptr = p.value

    def free(self):
        if self.ptr:
            F.lib().rt_device_free(self.ctx.handle, C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            if self.ptr and F._lib is not None and self.ctx.handle:
                self.free()
        except Exception:
            pass

    def to_numpy(self, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        F.check(F.lib().rt_memcpy_to_host(self.ctx.handle, out.ctypes.data, C.c_void_p(self.ptr), out.nbytes),
                self.ctx.handle)
        return out

    def from_numpy(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        F.check(F.lib().rt_memcpy_to_device(self.ctx.handle, C.c_void_p(self.ptr), arr.ctypes.data, arr.nbytes),
                self.ctx.handle)

    def zero(self):
        F.check(F.lib().rt_memset_device(self.ctx.handle, C.c_void_p(self.ptr), 0, self.nbytes), self.ctx.handle)


class Context:
    """One HIP device + stream + the device-resident scene (rt_ctx)."""

    def __init__(self, device=0):
        h = C.c_void_p()
        F.check(F.lib().rt_create(device, C.byref(h)))
        self._h = h
        self.device = device

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h and self._h.value:
            F.lib().rt_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            if F._lib is not None:
                self.close()
        except Exception:
            pass

    @staticmethod
    def device_count():
        n = C.c_int(0)
        rc = F.lib().rt_device_count(C.byref(n))
        return n.value if rc == F.RT_OK else 0

    def _chk(self, rc):
        return F.check(rc, self._h)

    def set_stream(self, hip_stream):
        self._chk(F.lib().rt_set_stream(self._h, _vp(hip_stream)))

    def synchronize(self):
        self._chk(F.lib().rt_synchronize(self._h))

    def set_option(self, opt, value):
        self._chk(F.lib().rt_set_option(self._h, opt, int(value)))

    def bsp_cull_in_use(self):
        """(mode, certified probe ms, silhouette probe ms): the culling mode the BSP
        kernels run now (rt_bsp_cull_in_use; RT_BSP_CULL_AUTO's choice once probed)."""
        m = C.c_int()
        ms = (C.c_float * 2)()
        self._chk(F.lib().rt_bsp_cull_in_use(self._h, C.byref(m), ms, None))
        return m.value, ms[0], ms[1]

    def bsp_cull_probes(self):
        """(probes started, probe launches) of RT_BSP_CULL_AUTO on this context
        (rt_bsp_cull_in_use's probes)."""
        m = C.c_int()
        n = (C.c_uint32 * 2)()
        self._chk(F.lib().rt_bsp_cull_in_use(self._h, C.byref(m), None, n))
        return n[0], n[1]

    def upload_mesh(self, mesh):
        self._chk(F.lib().rt_upload_mesh_host(self._h, mesh.handle))

    def upload_bsp(self, bsp):
        self._chk(F.lib().rt_upload_bsp_host(self._h, bsp.handle))

    def upload_bvh(self, bvh):
        self._chk(F.lib().rt_upload_bvh_host(self._h, bvh.handle))

    def build_bvh_device(self, max_prims=4):
        """HLBVH construction on the device from the uploaded mesh
        (hlbvh::Bvh::new + flatten + triangles, rt_build_bvh_device); becomes
        this context's BVH.  Returns the per-phase times (ms)."""
        t = F.BvhBuildTimes()
        self._chk(F.lib().rt_build_bvh_device(self._h, max_prims, C.byref(t)))
        return t.asdict()

    def build_bsp_device(self, max_depth=20, max_leaf=4):
        """BSP construction on the device from the uploaded mesh
        (BspTree::new + bsp_array + primitive_ids, rt_build_bsp_device);
        becomes this context's BSP.  Returns the phase times (ms)."""
        t = F.BspBuildTimes()
        self._chk(F.lib().rt_build_bsp_device(self._h, max_depth, max_leaf, C.byref(t)))
        return t.asdict()

    def download_bsp(self):
        """(tree[n,4] u32, planes[n] f32, ids[k] u32, aabb[8] f32) of this context's BSP."""
        nn, ni = C.c_uint32(), C.c_uint32()
        self._chk(F.lib().rt_download_bsp(self._h, None, None, 0, None, 0, None, C.byref(nn), C.byref(ni)))
        tree = np.zeros((max(1, nn.value), 4), np.uint32)
        planes = np.zeros(max(1, nn.value), np.float32)
        ids = np.zeros(max(1, ni.value), np.uint32)
        aabb = np.zeros(8, np.float32)
        self._chk(F.lib().rt_download_bsp(self._h, tree.ctypes.data_as(F.u32p), planes.ctypes.data_as(F.f32p),
                                          nn.value, ids.ctypes.data_as(F.u32p), ni.value,
                                          aabb.ctypes.data_as(F.f32p), C.byref(nn), C.byref(ni)))
        return tree[:nn.value], planes[:nn.value], ids[:ni.value], aabb

    def download_bsp_treelets(self, silhouette=False):
        """The BSP walk's 96-B treelets as u32[nnodes + 1, 24] (rt_download_bsp_treelets;
        diagnostics: the certified culling's per-subtree data); with silhouette=True
        also RT_BSP_CULL_SILHOUETTE's node data as u32[nnodes + 1, 4]."""
        nb = C.c_uint64()
        self._chk(F.lib().rt_download_bsp_treelets(self._h, None, 0, C.byref(nb)))
        out = np.zeros(nb.value // 4, np.uint32)
        self._chk(F.lib().rt_download_bsp_treelets(self._h, out.ctypes.data_as(C.c_void_p), nb.value, C.byref(nb)))
        w = F.BSP_TREELET_BYTES // 4
        slots = out.size // (w + 4)
        tl = out[:slots * w].reshape(-1, w)
        return (tl, out[slots * w:].reshape(-1, 4)) if silhouette else tl

    def download_bvh(self):
        """(nodes[n,8] u32 view of GpuNode, tri_ids[k] u32) of this context's BVH."""
        nn, ni = C.c_uint32(), C.c_uint32()
        self._chk(F.lib().rt_download_bvh(self._h, None, 0, None, 0, C.byref(nn), C.byref(ni)))
        nodes = (F.GpuNode * max(1, nn.value))()
        ids = np.zeros(max(1, ni.value), np.uint32)
        self._chk(F.lib().rt_download_bvh(self._h, nodes, nn.value, ids.ctypes.data_as(F.u32p), ni.value,
                                          C.byref(nn), C.byref(ni)))
        raw = np.frombuffer(nodes, dtype=np.uint32).reshape(-1, 8)[:nn.value].copy()
        return raw, ids[:ni.value].copy()

    def upload_mesh_arrays(self, vertices, normals, indices, materials, lights=None):
        pos = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 4)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 4)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 4)
        mats = np.ascontiguousarray(materials, dtype=np.float32).reshape(-1, 16)
        lp = None
        nl = 0
        if lights is not None:
            lights = np.ascontiguousarray(lights, dtype=np.uint32)
            lp, nl = F.as_u32p(lights), lights.shape[0]
        self._chk(F.lib().rt_upload_mesh(self._h, F.as_f32p(pos), F.as_f32p(nrm), pos.shape[0], F.as_u32p(idx),
                                         idx.shape[0], C.cast(mats.ctypes.data, C.POINTER(F.Material)),
                                         mats.shape[0], lp, nl))

    def upload_bsp_arrays(self, aabb, tree, planes, ids, max_depth):
        aabb = np.ascontiguousarray(aabb, dtype=np.float32)
        tree = np.ascontiguousarray(tree, dtype=np.uint32).reshape(-1, 4)
        planes = np.ascontiguousarray(planes, dtype=np.float32)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        self._chk(F.lib().rt_upload_bsp(self._h, F.as_f32p(aabb), F.as_u32p(tree), F.as_f32p(planes), tree.shape[0],
                                        F.as_u32p(ids), ids.shape[0], max_depth))

    def upload_bvh_arrays(self, nodes_u32x8, tri_ids):
        nodes = np.ascontiguousarray(nodes_u32x8, dtype=np.uint32).reshape(-1, 8)
        ids = np.ascontiguousarray(tri_ids, dtype=np.uint32)
        self._chk(F.lib().rt_upload_bvh(self._h, C.cast(nodes.ctypes.data, C.POINTER(F.GpuNode)), nodes.shape[0],
                                        F.as_u32p(ids), ids.shape[0]))

    def set_uniforms(self, uniform, jitter=None):
        jp = None
        if jitter is not None:
            self._jitter = np.ascontiguousarray(jitter, dtype=np.float32)
            jp = F.as_f32p(self._jitter)
        self._chk(F.lib().rt_set_uniforms(self._h, C.byref(uniform), jp))

    def set_environment(self, rgb):
        a = np.ascontiguousarray(rgb, dtype=np.float32)
        self._chk(F.lib().rt_set_environment(self._h, F.as_f32p(a)))

    def set_environment_map(self, rgba8):
        """hdri0 equirectangular background for W9E1: uint8[h, w, 4] (RGBA), or None."""
        if rgba8 is None:
            self._chk(F.lib().rt_set_environment_map(self._h, None, 0, 0))
            return
        a = np.ascontiguousarray(rgba8, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("environment map must be uint8[h, w, 4]")
        self._env_keep = a
        self._chk(F.lib().rt_set_environment_map(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1],
                                                 a.shape[0]))

    def set_texture(self, rgba8):
        """texture0 of the W3 scenes: uint8[h, w, 4] (RGBA, row 0 at v = 0), or None."""
        if rgba8 is None:
            self._chk(F.lib().rt_set_texture(self._h, None, 0, 0))
            return
        a = np.ascontiguousarray(rgba8, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("texture must be uint8[h, w, 4]")
        self._chk(F.lib().rt_set_texture(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0]))

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def render(self, mode, trav, region, first_iter, spp, accum_ptr, ids_ptr=None, counts=False):
        """rt_render on a region (x0, y0, w, h); device pointers in/out."""
        t = F.Tile(*region)
        cnt = F.RayCounts() if counts else None
        self._chk(F.lib().rt_render(self._h, F.MODES.get(mode, mode), F.TRAVERSALS.get(trav, trav), C.byref(t),
                                    first_iter, spp, C.c_void_p(accum_ptr), _vp(ids_ptr),
                                    C.byref(cnt) if counts else None))
        return cnt.asdict() if counts else None

    def render_tiles(self, mode, trav, rank, nranks, first_iter, spp, accum_ptr, ids_ptr=None, counts=False):
        ts = F.Tileset(rank, nranks)
        cnt = F.RayCounts() if counts else None
        self._chk(F.lib().rt_render_tiles(self._h, F.MODES.get(mode, mode), F.TRAVERSALS.get(trav, trav),
                                          C.byref(ts), first_iter, spp, C.c_void_p(accum_ptr),
                                          _vp(ids_ptr),
                                          C.byref(cnt) if counts else None))
        return cnt.asdict() if counts else None

    def unpack_tiles(self, width, height, nranks, packed_accum, packed_ids, frame_accum, frame_ids):
        self._chk(F.lib().rt_unpack_tiles(self._h, width, height, nranks, _vp(packed_accum), _vp(packed_ids),
                                          _vp(frame_accum), _vp(frame_ids)))

    # ---- the noise estimate of the path modes (include/rt.h "noise estimate")
    def set_noise_buffer(self, state_ptr=None):
        """rt_set_noise_buffer: the device buffer of rt_noise_state (8 B per output slot,
        indexed as accum) the path modes' renders update; None turns it off."""
        self._chk(F.lib().rt_set_noise_buffer(self._h, _vp(state_ptr)))

    def noise_accumulate(self, samples_ptr, npix, spp, pixel_major, first_iter, state_ptr):
        """rt_noise_accumulate: device records (float4) [pixel][iteration] (pixel_major) or
        [iteration][pixel] of iterations first_iter.. into the device state."""
        self._chk(F.lib().rt_noise_accumulate(self._h, C.c_void_p(samples_ptr), npix, spp, int(bool(pixel_major)),
                                              first_iter, C.c_void_p(state_ptr)))

    def noise_map(self, state_ptr, npix, n, floor, rel_ptr):
        """rt_noise_map: the relative standard error after n iterations per slot (device pointers)."""
        self._chk(F.lib().rt_noise_map(self._h, C.c_void_p(state_ptr), npix, n, float(floor), C.c_void_p(rel_ptr)))

    def noise_summary(self, state_ptr, npix, n, threshold, floor=1e-3):
        """rt_noise_summarize: {pixels, above, nonfinite, max_rel_err}; synchronizes."""
        s = F.NoiseSummary()
        self._chk(F.lib().rt_noise_summarize(self._h, C.c_void_p(state_ptr), npix, n, float(threshold), float(floor),
                                             C.byref(s)))
        return s.asdict()

    # ---- adaptive sampling of the path modes (include/rt.h "adaptive sampling")
    def set_adaptive(self, count_ptr=None, target=0.0, floor=1e-3, min_samples=16, vote="tile"):
        """rt_set_adaptive: the device buffer of per-slot sample counts (uint32, indexed as
        accum) and the rule's parameters; None turns it off."""
        self._chk(F.lib().rt_set_adaptive(self._h, _vp(count_ptr), float(target),
                                          float(floor), int(min_samples), F.ADAPT_VOTES.get(vote, vote)))

    def adaptive_accumulate(self, samples_ptr, npix, spp, pixel_major, first_iter, last_pass, live_ptr, accum_ptr,
                            ids_ptr, state_ptr, count_ptr):
        """rt_adaptive_accumulate: the fused fold of device records into the live pixels'
        accumulation, id, noise state and count (device pointers; live: one byte per pixel)."""
        self._chk(F.lib().rt_adaptive_accumulate(self._h, C.c_void_p(samples_ptr), npix, spp, int(bool(pixel_major)),
                                                 first_iter, int(bool(last_pass)), C.c_void_p(live_ptr),
                                                 C.c_void_p(accum_ptr), _vp(ids_ptr),
                                                 C.c_void_p(state_ptr), C.c_void_p(count_ptr)))

    def adaptive_map(self, state_ptr, count_ptr, npix, floor, rel_ptr):
        """rt_adaptive_map: the relative standard error per slot with n = the slot's count."""
        self._chk(F.lib().rt_adaptive_map(self._h, C.c_void_p(state_ptr), C.c_void_p(count_ptr), npix, float(floor),
                                          C.c_void_p(rel_ptr)))

    def adaptive_summary(self, state_ptr, count_ptr, width, height, iteration, target, floor=1e-3, min_samples=16,
                         vote="tile"):
        """rt_adaptive_summarize: {pixels, live_next, above, nonfinite, total_samples, min_count,
        max_count, max_rel_err} of a row-major width x height frame; synchronizes."""
        s = F.AdaptiveSummary()
        self._chk(F.lib().rt_adaptive_summarize(self._h, C.c_void_p(state_ptr), C.c_void_p(count_ptr), width, height,
                                                iteration, float(target), float(floor), int(min_samples),
                                                F.ADAPT_VOTES.get(vote, vote), C.byref(s)))
        return s.asdict()

    def adaptive_in_use(self):
        """rt_adaptive_in_use: {live, dealt, list} of the most recent path-mode render."""
        live, dealt, took = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        self._chk(F.lib().rt_adaptive_in_use(self._h, C.byref(live), C.byref(dealt), C.byref(took)))
        return {"live": int(live.value), "dealt": int(dealt.value), "list": bool(took.value)}

    # ---- the denoise filter (include/rt.h "denoise"; device pointers, asynchronous)
    def denoise_guide(self, width, height, ids_ptr, nz_ptr, dz_ptr, objects=0):
        """rt_denoise_guide: {N, z} (float4) and {dzx, dzy} (float2) per pixel from the primary ids,
        the uploaded mesh and the current uniforms; with objects (a mask of RT_GUIDE_*, see
        guide_objects_of()) rt_denoise_guide_objects: those analytic objects under the pixels without an id."""
        if objects:
            self._chk(F.lib().rt_denoise_guide_objects(self._h, int(objects), width, height, C.c_void_p(ids_ptr),
                                                       C.c_void_p(nz_ptr), C.c_void_p(dz_ptr)))
            return
        self._chk(F.lib().rt_denoise_guide(self._h, width, height, C.c_void_p(ids_ptr), C.c_void_p(nz_ptr),
                                           C.c_void_p(dz_ptr)))

    def denoise_variance(self, state_ptr, count_ptr, npix, n, var_ptr):
        """rt_denoise_variance: the variance of the mean luminance per slot, with the slot's own
        count (count_ptr) or n iterations (count_ptr None)."""
        self._chk(F.lib().rt_denoise_variance(self._h, C.c_void_p(state_ptr), _vp(count_ptr),
                                              npix, n, C.c_void_p(var_ptr)))

    def denoise_filter(self, width, height, color_ptr, var_ptr, nz_ptr, dz_ptr, out_color_ptr, out_var_ptr=None,
                       levels=5, sigma_l=4.0, sigma_z=1.0):
        """rt_denoise_filter: `levels` a-trous levels over colour and variance with the guide."""
        self._chk(F.lib().rt_denoise_filter(self._h, width, height, C.c_void_p(color_ptr), C.c_void_p(var_ptr),
                                            C.c_void_p(nz_ptr), C.c_void_p(dz_ptr), int(levels), float(sigma_l),
                                            float(sigma_z), C.c_void_p(out_color_ptr),
                                            _vp(out_var_ptr)))

    def denoise(self, width, height, accum_ptr, ids_ptr, state_ptr, count_ptr, n, out_ptr, levels=5, sigma_l=4.0,
                sigma_z=1.0, objects=0):
        """rt_denoise: guide, variance and filter of a rendered frame on the context's scratch; with
        objects (a mask of RT_GUIDE_*) rt_denoise_objects: the same with the guide of those objects."""
        if objects:
            self._chk(F.lib().rt_denoise_objects(self._h, int(objects), width, height, C.c_void_p(accum_ptr),
                                                 C.c_void_p(ids_ptr), C.c_void_p(state_ptr), _vp(count_ptr), int(n),
                                                 int(levels), float(sigma_l), float(sigma_z), C.c_void_p(out_ptr)))
            return
        self._chk(F.lib().rt_denoise(self._h, width, height, C.c_void_p(accum_ptr), C.c_void_p(ids_ptr),
                                     C.c_void_p(state_ptr), _vp(count_ptr), int(n),
                                     int(levels), float(sigma_l), float(sigma_z), C.c_void_p(out_ptr)))

    def denoise_level_times(self):
        """rt_denoise_level_times: ([ms per level], [form per level: 0 direct, 1 LDS tile, 2 lattice])
        of the most recent filter (RT_OPT_KERNEL_TIMING); synchronizes."""
        ms, form = (C.c_float * 5)(), (C.c_uint32 * 5)()
        self._chk(F.lib().rt_denoise_level_times(self._h, ms, form))
        return [float(x) for x in ms], [int(x) for x in form]

    # ---- temporal accumulation (include/rt.h "temporal accumulation"; device pointers, asynchronous)
    def temporal_accumulate(self, width, height, color_ptr, color_scale, nz_ptr, prev_uniform, hist, out,
                            max_history=32, normal_min=0.9, plane_tol=0.01):
        """rt_temporal_accumulate: the frame in color_ptr (x color_scale) blended with the history
        reprojected from prev_uniform's camera.  hist: (color, moments, length, nz) device pointers
        with prev_uniform, or None with None (a first frame); out: (color, moments, length)."""
        h = tuple(hist) if hist is not None else (None,) * 4
        self._chk(F.lib().rt_temporal_accumulate(
            self._h, width, height, _vp(color_ptr), float(color_scale), _vp(nz_ptr),
            C.byref(prev_uniform) if prev_uniform is not None else None, _vp(h[0]), _vp(h[1]), _vp(h[2]), _vp(h[3]),
            int(max_history), float(normal_min), float(plane_tol), _vp(out[0]), _vp(out[1]), _vp(out[2])))

    def temporal_variance(self, width, height, mom_ptr, len_ptr, nz_ptr, dz_ptr, var_ptr, min_len=4, normal_min=0.9,
                          plane_tol=0.01):
        """rt_temporal_variance: the variance of the integrated mean luminance; a pixel with fewer
        than min_len frames takes its 7 x 7 neighbours' moments."""
        self._chk(F.lib().rt_temporal_variance(self._h, width, height, _vp(mom_ptr), _vp(len_ptr), _vp(nz_ptr),
                                               _vp(dz_ptr), int(min_len), float(normal_min), float(plane_tol),
                                               _vp(var_ptr)))

    def temporal_times(self):
        """rt_temporal_times: (accumulate ms, variance ms, variance form: 0 direct, 1 LDS tile) of the
        most recent calls (RT_OPT_KERNEL_TIMING); synchronizes."""
        a, v, f = C.c_float(0), C.c_float(0), C.c_uint32(0)
        self._chk(F.lib().rt_temporal_times(self._h, C.byref(a), C.byref(v), C.byref(f)))
        return float(a.value), float(v.value), int(f.value)

    # ---- the tile gather over RCCL (include/rt.h "multi-GPU")
    @staticmethod
    def comm_unique_id():
        """rt_comm_unique_id: a new communicator id (bytes, RT_COMM_ID_BYTES)."""
        buf = (C.c_uint8 * F.RT_COMM_ID_BYTES)()
        F.check(F.lib().rt_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, nranks, rank, uid):
        """rt_comm_init: join communicator `uid` as `rank` of `nranks` (collective)."""
        buf = (C.c_uint8 * F.RT_COMM_ID_BYTES).from_buffer_copy(uid)
        self._chk(F.lib().rt_comm_init(self._h, nranks, rank, buf))

    def comm_destroy(self):
        self._chk(F.lib().rt_comm_destroy(self._h))

    def gather_tiles(self, width, height, local_accum, local_ids, frame_accum=None, frame_ids=None):
        """rt_gather_tiles: every rank's packed tiles to rank 0's frame (device pointers)."""
        self._chk(F.lib().rt_gather_tiles(self._h, width, height, _vp(local_accum), _vp(local_ids), _vp(frame_accum),
                                          _vp(frame_ids)))

    def trace_rays(self, trav, rays, anyhit=None):
        """rt_trace_rays on host arrays: rays float32[n, 8] (origin, direction,
        tmin, tmax), anyhit bool[n] or None.  Returns a structured array with the
        fields of rt_ray_hit (tri, dist, beta, gamma, ntested, tested_fnv, tmin, tmax)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        out = np.zeros(n, dtype=RAY_HIT_DTYPE)
        if n == 0:
            return out
        rb = self.alloc(rays.nbytes)
        hb = self.alloc(out.nbytes)
        fb = None
        try:
            rb.from_numpy(rays)
            if anyhit is not None:
                fb = self.alloc(4 * n)
                fb.from_numpy(np.ascontiguousarray(np.asarray(anyhit).astype(np.uint32)))
            self._chk(F.lib().rt_trace_rays(self._h, F.TRAVERSALS.get(trav, trav), C.c_void_p(rb.ptr),
                                            C.c_void_p(fb.ptr) if fb else None, n, C.c_void_p(hb.ptr)))
            return hb.to_numpy(RAY_HIT_DTYPE, (n,))
        finally:
            for b in (rb, hb, fb):
                if b is not None:
                    b.free()

    def last_counts(self):
        cnt = F.RayCounts()
        self._chk(F.lib().rt_last_counts(self._h, C.byref(cnt)))
        return cnt.asdict()

    def last_elided_shadows(self):
        """Shadow rays of the last launch that were resolved at shading time, not walked
        (rt_last_elided_shadows); 0 unless the detail counters are on."""
        n = C.c_uint64()
        self._chk(F.lib().rt_last_elided_shadows(self._h, C.byref(n)))
        return n.value

    def last_elided_primaries(self):
        """Camera rays of the last render that RT_OPT_EMPTY_PIXELS did not cast
        (rt_last_elided_primaries): its flagged pixels x its iterations."""
        n = C.c_uint64()
        self._chk(F.lib().rt_last_elided_primaries(self._h, C.byref(n)))
        return n.value

    def empty_pixels_in_use(self):
        """(pixels flagged, build ms) of the empty-pixel mask the last render used
        (rt_empty_pixels_in_use); 0 pixels when it used none."""
        n = C.c_uint64()
        ms = C.c_float()
        self._chk(F.lib().rt_empty_pixels_in_use(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def download_empty_mask(self, width, height):
        """The last render's empty-pixel mask as a (height, width) bool array
        (rt_download_empty_mask); all False when it used none."""
        words = np.zeros((width * height + 31) // 32, np.uint32)
        self._chk(F.lib().rt_download_empty_mask(self._h, F.as_u32p(words), words.size))
        return _mask_bits(words, width, height)

    def last_pixel_depth(self, width, height):
        """(near, far, in use) of the pixel depth ranges the last render's camera rays
        started on (rt_last_pixel_depth): two (height, width) float32 arrays; near 0 and
        far +inf everywhere, and in use False, when it used none."""
        near = np.empty(width * height, np.float32)
        far = np.empty(width * height, np.float32)
        used = C.c_int()
        self._chk(F.lib().rt_last_pixel_depth(self._h, F.as_f32p(near), F.as_f32p(far), near.size, C.byref(used)))
        return near.reshape(height, width), far.reshape(height, width), bool(used.value)

    def timer_start(self):
        self._chk(F.lib().rt_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float()
        self._chk(F.lib().rt_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def frame_rgba8(self, accum_ptr, npix, out_ptr, mode=None):
        """Display transform of npix accumulated pixels into 8-bit sRGB RGBA (device pointers).
        mode: the rt_mode that rendered them (rt_frame_rgba8_mode: W1E2 and W1E3 are
        displayed without the pow); None: rt_frame_rgba8."""
        if mode is None:
            self._chk(F.lib().rt_frame_rgba8(self._h, C.c_void_p(accum_ptr), npix, C.c_void_p(out_ptr)))
        else:
            self._chk(F.lib().rt_frame_rgba8_mode(self._h, F.MODES.get(mode, mode), C.c_void_p(accum_ptr), npix,
                                                  C.c_void_p(out_ptr)))

    def kernel_time(self, reset=True):
        """(summed ms, launches) of the traversal-kernel launches timed since the
        last reset (RT_OPT_KERNEL_TIMING must be on); synchronizes."""
        ms = C.c_double()
        n = C.c_uint32()
        self._chk(F.lib().rt_kernel_time(self._h, int(reset), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def trace_batch(self, trav, rays_ptr, flags_ptr, n, hits_ptr):
        """rt_trace_batch: the traversal-only kernel over n device rays (8 f32 each;
        flags bit 0 any-hit, or None) into n x {record offset | 0xFFFFFFFE | ~0, dist}."""
        self._chk(F.lib().rt_trace_batch(self._h, F.TRAVERSALS.get(trav, trav), C.c_void_p(rays_ptr),
                                          _vp(flags_ptr), n, C.c_void_p(hits_ptr)))

    def set_ray_capture(self, rays_ptr=None, flags_ptr=None, cap=0):
        """Arm (device buffers of cap rays) or disarm (None) the counting renders' ray capture."""
        self._chk(F.lib().rt_set_ray_capture(self._h, _vp(rays_ptr),
                                              _vp(flags_ptr), cap))

    def ray_capture_count(self):
        n = C.c_uint64()
        self._chk(F.lib().rt_ray_capture_count(self._h, C.byref(n)))
        return n.value

    def gather_time(self, reset=True):
        """(transfer ms, unpack ms, calls) of the frame assembly timed since the last
        reset (rt_gather_time: rt_gather_tiles' RCCL transfers and every unpack;
        RT_OPT_KERNEL_TIMING must be on); synchronizes."""
        tx = C.c_double()
        up = C.c_double()
        n = C.c_uint32()
        self._chk(F.lib().rt_gather_time(self._h, int(reset), C.byref(tx), C.byref(up), C.byref(n)))
        return tx.value, up.value, n.value

    def selftest_math(self, n=1 << 20, lo=-4.0, hi=4.0):
        bad = C.c_uint32()
        self._chk(F.lib().rt_selftest_math(self._h, n, lo, hi, C.byref(bad)))
        return bad.value


def guide_objects_of(mode):
    """rt_guide_objects: the mask (RT_GUIDE_*) of the analytic objects a mode's shader tests
    beside the mesh and that leave no primary id; mode: a name or an rt_mode value."""
    out = C.c_uint32(0)
    F.check(F.lib().rt_guide_objects(F.MODES[mode] if isinstance(mode, str) else int(mode), C.byref(out)))
    return int(out.value)


def _mask_bits(words, width, height):
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:width * height]
    return bits.reshape(height, width).astype(bool)


def empty_mask_host(mesh, uniform):
    """The empty-pixel mask of RT_OPT_EMPTY_PIXELS computed on the host, no device
    (rt_empty_mask_host): a (height, width) bool array, True = no camera ray of the
    pixel can hit the mesh.  The device mask of the same mesh and uniforms is the same bits."""
    V, _, I, _, _ = mesh.arrays()
    V = np.ascontiguousarray(V, np.float32)
    I = np.ascontiguousarray(I, np.uint32)
    W, H = int(uniform.resolution[0]), int(uniform.resolution[1])
    words = np.zeros((W * H + 31) // 32, np.uint32)
    n = C.c_uint64()
    F.check(F.lib().rt_empty_mask_host(F.as_f32p(V), V.shape[0], F.as_u32p(I), I.shape[0], C.byref(uniform),
                                       F.as_u32p(words), C.byref(n)))
    return _mask_bits(words, W, H)


def pixel_depth_host(mesh, uniform):
    """The per-pixel depth ranges of RT_OPT_PIXEL_DEPTH computed on the host, no device
    (rt_pixel_depth_host): (near, far), two (height, width) float32 arrays that bound,
    strictly, every distance a camera ray of the pixel can be accepted with; near +inf and
    far 0 for a pixel empty_mask_host flags.  The device arrays are the same bits."""
    V, _, I, _, _ = mesh.arrays()
    V = np.ascontiguousarray(V, np.float32)
    I = np.ascontiguousarray(I, np.uint32)
    W, H = int(uniform.resolution[0]), int(uniform.resolution[1])
    near = np.empty(W * H, np.float32)
    far = np.empty(W * H, np.float32)
    F.check(F.lib().rt_pixel_depth_host(F.as_f32p(V), V.shape[0], F.as_u32p(I), I.shape[0], C.byref(uniform),
                                        F.as_f32p(near), F.as_f32p(far)))
    return near.reshape(H, W), far.reshape(H, W)


def load_texture_rgba8(path):
    """Texture::from_file (src/bindings/texture.rs:98, image.to_rgba8()): a
    JPEG/PNG as uint8[h, w, 4].  Decoded with PIL (the reference's image 0.24
    decoder is not available: texel values are parity-unpinned)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGBA"), dtype=np.uint8).copy()


def synth_texture(size=64):
    """Deterministic stand-in for res/textures/grass.jpg (not redistributed): uint8
    [size, size, 4], mottled greens from an integer hash of the texel coordinates
    (the same arithmetic as raytracer::synth_texture, include/raytracer.hpp)."""
    y, x = np.meshgrid(np.arange(size, dtype=np.uint32), np.arange(size, dtype=np.uint32), indexing="ij")
    h = (x * np.uint32(73856093)) ^ (y * np.uint32(19349663))
    h = (h ^ (h >> np.uint32(13))) * np.uint32(0x5BD1E995)
    h = h ^ (h >> np.uint32(15))
    t = np.empty((size, size, 4), np.uint8)
    t[..., 0] = 40 + (h & np.uint32(63))
    t[..., 1] = 120 + ((h >> np.uint32(8)) & np.uint32(127))
    t[..., 2] = 20 + ((h >> np.uint32(16)) & np.uint32(31))
    t[..., 3] = 255
    return t


def local_tiles(width, height, nranks):
    return int(F.lib().rt_tileset_local_tiles(width, height, nranks))
