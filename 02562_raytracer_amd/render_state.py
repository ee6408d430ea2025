"""Headless RenderState: mirror of src/render_state.rs (setup_rendering
:161-265, update :467-481, render :483-561) and of the progressive loop of
src/lib.rs:321-363, on top of the C ABI.

Differences from the windowed reference, all deliberate:
  * no window/surface: aspect = W/H of SceneDescriptor.res (the reference
    uses the window's inner size, render_state.rs:563-566);
  * the accumulation "texture" is an HBM float4 array (linear RGBA32F), and
    the display transform pow(., 1.5) is left to the caller;
  * the W9E1 equirectangular hdri0 is the scene's background_hdri texture
    when the file is in assets/textures (decoded with PIL, sampled as
    include/rt_detmath.h pins it), else a constant environment colour;
  * a missing bunny.obj can be replaced by the deterministic stand-in
    (bunny_standin=True), since the reference checkout lacks it;
  * texture0 of the W3 scenes is assets/textures/grass.jpg when a user has put
    it there (the reference's file is not redistributed), else the
    deterministic stand-in core.synth_texture().
"""
import os

import numpy as np

from . import _ffi as F
from .camera import Camera, CameraController
from .jitter import MAX_SUBDIVISION, jitters_for
from .core import BspTree, Bvh, Context, Mesh, guide_objects_of, make_uniform, synth_texture

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(REPO, "assets", "models")


class RenderState:
    guide_objects = False   # set_guide_objects(): the guide also sees the mode's analytic objects

    def __init__(self, scene, device=0, ctx=None, models_dir=ASSETS, bunny_standin=True, selection1=0,
                 env=(1.0, 1.0, 1.0), resolution=None, device_build=False):
        self.ctx = ctx if ctx is not None else Context(device)
        self.models_dir = models_dir
        self.bunny_standin = bunny_standin
        self.selection1 = selection1
        self.selection2 = 0          # Uniform defaults, uniform.rs:152-156
        self.use_texture = 0
        self.uv_scale = (1.0, 1.0)
        self.env = env
        self.resolution = resolution
        self.device_build = device_build   # build the BSP / HLBVH on the GPU (same arrays)
        self.progressive = True
        self.iteration = 0
        self.max_iterations = 2   # Uniform::max_iterations, SetSamples (lib.rs:472-479)
        self.subdivision_level = 1   # Uniform.subdivision_level (uniform.rs:122-129)
        self.camera_controller = CameraController()
        self.noise = None   # enable_noise(): the device buffer of rt_noise_state
        self.counts = None  # enable_adaptive(): the device buffer of per-pixel sample counts
        self.adaptive = None   # its parameters: target, floor, min_samples, vote
        self.temporal = None   # enable_temporal(): its buffers, parameters and frame counter
        self.setup_rendering(scene)

    def _background(self, scene):
        """render_state.rs:191-206: the scene's background_hdri, if present."""
        if not getattr(scene, "background_hdri", None):
            return None
        path = os.path.join(REPO, "assets", "textures", os.path.basename(scene.background_hdri))
        if not os.path.exists(path):
            return None
        from .core import load_texture_rgba8
        return load_texture_rgba8(path)

    def _texture0(self):
        """render_state.rs:176-189: texture0 (grass.jpg), or its stand-in."""
        path = os.path.join(REPO, "assets", "textures", "grass.jpg")
        if os.path.exists(path):
            from .core import load_texture_rgba8
            return load_texture_rgba8(path)
        return synth_texture()

    # render_state.rs:161-265
    def setup_rendering(self, scene):
        row = F.MODE_OF_SHADER.get(scene.shader)   # (its name is scene.kernel_mode)
        if row is None:
            raise F.RtError(F.RT_E_UNSUPPORTED, f"{scene.shader} is outside the hot path (SURVEY.md section 2)")
        self.scene = scene
        self.camera = Camera.from_tuple(scene.camera)
        self.mode = row.name
        self.width, self.height = self.resolution or scene.res
        self.mesh = self.bsp = self.bvh = None
        self.trav = scene.traverse_type if row.family in F.TREE_FAMILIES else "NONE"
        if row.flags & F.RT_MODEF_TEXTURE0:
            self.ctx.set_texture(self._texture0())   # the W3 scenes sample texture0
        elif row.family == F.RT_FAMILY_ANALYTIC:
            self.ctx.set_texture(None)
        if row.family in F.MESH_FAMILIES:
            self.mesh = self._load_model(scene.model)
            self.ctx.upload_mesh(self.mesh)
            if self.trav == "BSP":
                if self.device_build:
                    self.ctx.build_bsp_device(20, 4)
                else:
                    self.bsp = self.mesh.bsp_tree()   # Mesh::bsp_tree, mesh.rs:229-231 (depth 20, leaf 4)
                    self.ctx.upload_bsp(self.bsp)
            elif self.trav == "BVH":   # ("NONE": the brute-force W5 scenes, the mesh alone)
                if self.device_build:
                    self.ctx.build_bvh_device(4)
                else:
                    self.bvh = self.mesh.bvh()        # Mesh::bvh, mesh.rs:233-239 (leaf 4)
                    self.ctx.upload_bvh(self.bvh)
        self.ctx.set_environment(self.env)
        self.ctx.set_environment_map(None)
        tex = self._background(scene)
        if tex is not None:
            self.ctx.set_environment_map(tex)
        npx = self.width * self.height
        self.accum = self.ctx.alloc(npx * 16)
        self.accum.zero()
        self.ids = self.ctx.alloc(npx * 4)
        self.iteration = 0
        adaptive = self.adaptive
        if adaptive is not None:
            self.disable_adaptive()
        if self.noise is not None:
            # the noise buffer follows the scene: a new one for a path mode, none otherwise
            self.disable_noise()
            if self.mode in F.NOISE_MODES:
                self.enable_noise()
        if adaptive is not None and self.mode in F.NOISE_MODES:
            self.enable_adaptive(**adaptive)   # and so do the sample counts
        temporal = self.temporal
        if temporal is not None:
            # ... and the temporal buffers: a new sequence for a path mode, none otherwise
            self.disable_temporal()
            if self.mode in F.NOISE_MODES:
                self.enable_temporal(min_len=temporal["min_len"], **temporal["params"])
        self.update()

    def _load_model(self, model):
        path = os.path.join(self.models_dir, model)
        if not os.path.exists(path) and model == "bunny.obj" and self.bunny_standin:
            return Mesh.synth_bunny()
        return Mesh.from_obj(path)

    def load_scene(self, scene):
        """RenderState::load_scene (render_state.rs:314-334): full rebuild;
        the iteration restarts (Command::LoadScene, lib.rs:464-469)."""
        self.iteration = 0
        self.setup_rendering(scene)

    # render_state.rs:467-481: the controller moves the camera, then the uniform follows
    def update(self):
        self.camera.aspect = float(np.float32(self.width) / np.float32(self.height))
        self.camera_controller.update_camera(self.camera)
        eye, target, up, constant = self.camera.as_args()
        self.uniform = make_uniform(eye, target, up, constant, self.width, self.height,
                                    selection1=self.selection1, iteration=self.iteration,
                                    subdiv=self.subdivision_level, selection2=self.selection2,
                                    use_texture=self.use_texture, uv_scale=self.uv_scale)
        # UniformGpu::update_buffer (uniform.rs:163-175): the jitter table with the uniforms
        self.ctx.set_uniforms(self.uniform, jitters_for(self.height, self.subdivision_level))

    def set_subdivision_level(self, level):
        """Uniform::update_subdivision_level (uniform.rs:122-129): clamped to 10;
        W6E1/PROJECT take level^2 stratified samples per pixel."""
        self.subdivision_level = min(int(level), MAX_SUBDIVISION)

    def set_sphere_material(self, shader):
        """Command::SetSphereMaterial (lib.rs:404-408): selection1, at the next update()."""
        self.selection1 = int(shader)

    def set_other_material(self, shader):
        """Command::SetOtherMaterial (lib.rs:409-411): selection2, at the next update()."""
        self.selection2 = int(shader)

    def set_texture(self, use, uv_scale):
        """Command::SetTexture (lib.rs:415-421): use_texture and uv_scale, at the next update()."""
        self.use_texture = int(use)
        self.uv_scale = (float(uv_scale[0]), float(uv_scale[1]))

    def input(self, key, pressed=True):
        """RenderState::input_alt (render_state.rs:462-465): a key event for the
        camera controller; takes effect at the next update()."""
        return self.camera_controller.handle_camera_commands(key, pressed)

    def set_camera_constant(self, constant):
        """Command::SetCameraConstant (lib.rs:401-403)."""
        self.camera.constant = float(constant)

    def set_samples(self, samples, enabled):
        """Command::SetSamples (lib.rs:472-479): progressive rendering up to
        `samples` iterations, or (disabled) a frame per step at a fixed iteration."""
        self.progressive = bool(enabled)
        self.max_iterations = int(samples) if enabled else 2

    def step(self):
        """One pass of rendering_thread (lib.rs:331-363): render while
        progressive and below max_iterations (or always when not progressive),
        advance the iteration when progressive, then update().  Returns whether
        a frame was rendered."""
        if self.progressive and self.iteration >= self.max_iterations:
            return False
        self.render(1)
        return True

    # render_state.rs:483-561 (+ lib.rs:349-354 iteration advance)
    def render(self, spp=1, counts=False):
        first = self.iteration   # not progressive: the iteration stays (lib.rs:350-355)
        c = self.ctx.render(self.mode, self.trav, (0, 0, self.width, self.height), first, spp, self.accum.ptr,
                            self.ids.ptr, counts=counts)
        if self.progressive and self.mode in F.PATH_MODES:
            self.iteration += spp
        self.update()
        return c

    def reset_iteration(self):
        self.iteration = 0
        self.update()

    # ---- the noise estimate (include/rt.h "noise estimate"; single process, no tiles)
    def enable_noise(self):
        """Keep the per-pixel running mean and variance of the iterations' luminance
        (rt_set_noise_buffer) from iteration 0 on; reallocated by load_scene."""
        if self.mode not in F.NOISE_MODES:
            raise ValueError(f"{self.mode} writes no per-iteration records: the noise estimate follows "
                             f"{', '.join(F.NOISE_MODES)}")
        if self.iteration:
            raise ValueError("enable_noise: the estimate starts at iteration 0 (reset_iteration() first)")
        if self.noise is None:
            self.noise = self.ctx.alloc(self.width * self.height * 8)
            self.noise.zero()
        self.ctx.set_noise_buffer(self.noise.ptr)

    def disable_noise(self):
        if self.counts is not None:
            self.disable_adaptive()   # (a count buffer without a noise buffer renders nothing)
        self.ctx.set_noise_buffer(None)
        if self.noise is not None:
            self.noise.free()   # (rt_device_free waits for the renders that wrote it)
            self.noise = None

    def _noise_or_raise(self):
        if self.noise is None:
            raise ValueError("no noise buffer: enable_noise() before the first iteration")
        return self.noise.ptr

    def noise_map(self, floor=1e-3):
        """The relative standard error of every pixel's mean luminance after the
        iterations rendered so far (at least 2): float32 [H, W], NaN where a sample was
        not finite (rt_noise_map)."""
        npx = self.width * self.height
        out = self.ctx.alloc(npx * 4)
        try:
            self.ctx.noise_map(self._noise_or_raise(), npx, self.iteration, floor, out.ptr)
            return out.to_numpy(np.float32, (self.height, self.width))
        finally:
            out.free()

    def noise_summary(self, threshold, floor=1e-3):
        """{pixels, above, nonfinite, max_rel_err} of the frame (rt_noise_summarize): above
        counts the finite pixels whose relative standard error exceeds threshold."""
        return self.ctx.noise_summary(self._noise_or_raise(), self.width * self.height, self.iteration, threshold,
                                      floor)

    def render_until(self, target, max_samples, batch=16, allow=0.0, floor=1e-3):
        """Render `batch` iterations at a time (the last batch clipped to max_samples)
        until at most allow x pixels lie above the relative standard error `target`, or
        max_samples iterations are done.  Returns (iterations, summary); the summary is
        None when fewer than 2 iterations were rendered."""
        if not self.progressive:
            raise ValueError("render_until needs progressive rendering (set_samples(.., True))")
        if batch < 1:
            raise ValueError("render_until: batch must be at least 1")
        if self.noise is None:
            self.enable_noise()
        summary = None
        while self.iteration < max_samples:
            self.render(min(int(batch), int(max_samples) - self.iteration))
            if self.iteration >= 2:
                summary = self.noise_summary(target, floor)
                if summary["above"] <= allow * summary["pixels"]:
                    break
        return self.iteration, summary

    # ---- adaptive sampling (include/rt.h "adaptive sampling"; single process, no tiles)
    def enable_adaptive(self, target, floor=1e-3, min_samples=16, vote="tile"):
        """Render only the pixels that have not converged: a pixel (vote "pixel") or an 8x8
        tile (vote "tile", the default) stops taking samples once it has min_samples
        iterations and its relative standard error is at most target (rt_set_adaptive).
        Enables the noise estimate if needed; starts at iteration 0; reallocated by
        load_scene."""
        if vote not in F.ADAPT_VOTES:
            raise ValueError(f"enable_adaptive: vote must be one of {', '.join(F.ADAPT_VOTES)}")
        if int(min_samples) < 2:
            raise ValueError("enable_adaptive: min_samples must be at least 2")
        if not float(target) >= 0.0:
            raise ValueError("enable_adaptive: target must be >= 0")
        if not float(floor) > 0.0:
            raise ValueError("enable_adaptive: floor must be > 0")
        if self.iteration:
            raise ValueError("enable_adaptive: the counts start at iteration 0 (reset_iteration() first)")
        if self.noise is None:
            self.enable_noise()
        if self.counts is None:
            self.counts = self.ctx.alloc(self.width * self.height * 4)
            self.counts.zero()
        self.adaptive = {"target": float(target), "floor": float(floor), "min_samples": int(min_samples), "vote": vote}
        self.ctx.set_adaptive(self.counts.ptr, **self.adaptive)

    def disable_adaptive(self):
        self.ctx.set_adaptive(None)
        if self.counts is not None:
            self.counts.free()
            self.counts = None
        self.adaptive = None

    def _adaptive_or_raise(self):
        if self.counts is None:
            raise ValueError("adaptive sampling is off: enable_adaptive() before the first iteration")
        return self.counts.ptr

    def sample_counts(self):
        """The iterations folded into every pixel: uint32 [H, W]."""
        self._adaptive_or_raise()
        return self.counts.to_numpy(np.uint32, (self.height, self.width))

    def adaptive_summary(self):
        """{pixels, live_next, above, nonfinite, total_samples, min_count, max_count,
        max_rel_err} of the frame (rt_adaptive_summarize): every pixel's error with its own
        count; live_next = the pixels the next render would sample."""
        counts = self._adaptive_or_raise()
        return self.ctx.adaptive_summary(self._noise_or_raise(), counts, self.width, self.height, self.iteration,
                                         **self.adaptive)

    def render_adaptive(self, max_samples, batch=16):
        """Render `batch` iterations at a time (the last batch clipped to max_samples) until
        no pixel is live any more or max_samples iterations are done.  Returns (iterations,
        summary); the summary is None when nothing was rendered."""
        self._adaptive_or_raise()
        if not self.progressive:
            raise ValueError("render_adaptive needs progressive rendering (set_samples(.., True))")
        if batch < 1:
            raise ValueError("render_adaptive: batch must be at least 1")
        summary = None
        while self.iteration < max_samples:
            self.render(min(int(batch), int(max_samples) - self.iteration))
            summary = self.adaptive_summary()
            if summary["live_next"] == 0:
                break
        return self.iteration, summary

    def _filtered_frame(self, fill, rgba8):
        """What the four filtered-frame methods share: fill(out) writes a float4 frame into a device
        buffer; returned as float32 [H, W, 4], or (rgba8) through rt_frame_rgba8_mode as uint8
        [H, W, 4].  The buffers are freed whatever happens."""
        npx = self.width * self.height
        bufs = []
        try:
            bufs.append(self.ctx.alloc(npx * 16))
            if rgba8:
                bufs.append(self.ctx.alloc(npx * 4))
            fill(bufs[0])
            if not rgba8:
                return bufs[0].to_numpy(np.float32, (self.height, self.width, 4))
            self.ctx.frame_rgba8(bufs[0].ptr, npx, bufs[1].ptr, mode=self.mode)
            return bufs[1].to_numpy(np.uint8, (self.height, self.width, 4))
        finally:
            for b in bufs:
                b.free()

    # ---- the guide with objects (include/rt.h "denoise / Guide with objects")
    def set_guide_objects(self, on):
        """Off (the default): the guide of denoise(), denoised_rgba8(), temporal_step(),
        temporal_frame() and temporal_rgba8() is rt_denoise_guide's, for which the W8 balls and
        the W9E2 / W9E3 holdout plane are background.  On: it is rt_denoise_guide_objects' with
        rt_guide_objects(mode), which gives those pixels the object's normal and depth -- and a
        history; a mode without such objects is not changed.  A history's guide must come from
        one definition: set it before enable_temporal().  load_scene keeps it."""
        if getattr(self, "temporal", None) is not None:
            raise ValueError("set_guide_objects: temporal accumulation is enabled and its history holds the guide "
                             "it was made with (set_guide_objects before enable_temporal)")
        self.guide_objects = bool(on)

    def _guide_mask(self):
        """the objects mask of the guides this state makes (0: rt_denoise_guide and rt_denoise themselves)"""
        return guide_objects_of(self.mode) if self.guide_objects else 0

    # ---- the denoise filter (include/rt.h "denoise"; single process, no tiles)
    def _denoise_check(self, levels, sigma_l, sigma_z):
        """(no device: the checks come before any allocation)"""
        if self.mode not in F.NOISE_MODES:
            raise ValueError(f"{self.mode} keeps no noise state: the denoise filter follows {', '.join(F.NOISE_MODES)}")
        self._noise_or_raise()
        if self.iteration < 2:
            raise ValueError("denoise: the variance needs at least 2 rendered iterations")
        if not 1 <= int(levels) <= 5:
            raise ValueError("denoise: levels must be in 1..5")
        if not (float(sigma_l) > 0.0 and float(sigma_z) > 0.0):
            raise ValueError("denoise: the sigmas must be > 0")

    def _denoise_into(self, out, levels, sigma_l, sigma_z):
        state = self._noise_or_raise()
        counts = self.counts.ptr if self.counts is not None else None
        self.ctx.denoise(self.width, self.height, self.accum.ptr, self.ids.ptr, state, counts, self.iteration, out.ptr,
                         levels=levels, sigma_l=sigma_l, sigma_z=sigma_z, objects=self._guide_mask())

    def denoise(self, levels=5, sigma_l=4.0, sigma_z=1.0):
        """The frame through the variance-guided a-trous filter (rt_denoise): float32 [H, W, 4],
        alpha 1.  Needs enable_noise() from iteration 0 and at least 2 iterations; with adaptive
        sampling every pixel's variance uses its own sample count.  The accumulation, the ids and
        the noise state are not changed."""
        self._denoise_check(levels, sigma_l, sigma_z)
        return self._filtered_frame(lambda out: self._denoise_into(out, levels, sigma_l, sigma_z), rgba8=False)

    def denoised_rgba8(self, levels=5, sigma_l=4.0, sigma_z=1.0):
        """The denoised frame as the sRGB surface would hold it: uint8 [H, W, 4]
        (rt_frame_rgba8_mode of denoise())."""
        self._denoise_check(levels, sigma_l, sigma_z)
        return self._filtered_frame(lambda out: self._denoise_into(out, levels, sigma_l, sigma_z), rgba8=True)

    # ---- temporal accumulation (include/rt.h "temporal accumulation"; single process, no tiles)
    def enable_temporal(self, max_history=32, normal_min=0.9, plane_tol=0.01, min_len=4):
        """Frames that follow a moving camera: temporal_step() renders a frame of its own and
        blends it with the history reprojected from the previous camera; temporal_frame() filters
        the result.  Allocates the current frame's accumulation and ids, a guide and two history
        sets; the progressive accum, ids, iteration, noise and adaptive state are not touched.
        Reallocated by load_scene."""
        if self.mode not in F.NOISE_MODES:
            raise ValueError(f"{self.mode} writes no per-iteration records: temporal accumulation follows "
                             f"{', '.join(F.NOISE_MODES)}")
        if int(max_history) < 1 or int(min_len) < 1:
            raise ValueError("enable_temporal: max_history and min_len must be at least 1")
        if not float(plane_tol) >= 0.0 or float(normal_min) != float(normal_min):
            raise ValueError("enable_temporal: plane_tol must be >= 0 and normal_min a number")
        if getattr(self, "temporal", None) is not None:
            self.disable_temporal()
        npx = self.width * self.height
        bufs = []

        def alloc(nbytes):
            bufs.append(self.ctx.alloc(nbytes))
            return bufs[-1]
        try:
            sets = [{"color": alloc(npx * 16), "mom": alloc(npx * 8), "len": alloc(npx * 4), "nz": alloc(npx * 16)}
                    for _ in range(2)]
            cur, ids, dz = alloc(npx * 16), alloc(npx * 4), alloc(npx * 8)
        except Exception:
            for b in bufs:   # a failed allocation leaves the state off, with nothing held
                b.free()
            raise
        self.temporal = {"params": {"max_history": int(max_history), "normal_min": float(normal_min),
                                    "plane_tol": float(plane_tol)}, "min_len": int(min_len),
                         "cur": cur, "ids": ids, "dz": dz, "sets": sets, "latest": None, "uniform": None, "k": 0}

    def disable_temporal(self):
        t, self.temporal = self.temporal, None
        if t is not None:
            for b in [t["cur"], t["ids"], t["dz"]] + [b for s in t["sets"] for b in s.values()]:
                b.free()

    def _temporal_or_raise(self, stepped=False):
        if self.temporal is None:
            raise ValueError("temporal accumulation is off: enable_temporal() first")
        if stepped and self.temporal["latest"] is None:
            raise ValueError("no temporal frame yet: temporal_step() first")
        return self.temporal

    def temporal_step(self, spp=1):
        """One frame of the sequence: spp iterations from the sequence's own counter into a zeroed
        buffer, its guide, the blend with the reprojected history (rt_temporal_accumulate), then
        update() -- which moves the camera for the next frame."""
        t = self._temporal_or_raise()
        if int(spp) < 1:
            raise ValueError("temporal_step: spp must be at least 1")
        w, h, k = self.width, self.height, t["k"]
        t["cur"].zero()
        # the frame is not the progressive render's: its noise state and counts stay as they are
        if self.counts is not None:
            self.ctx.set_adaptive(None)
        if self.noise is not None:
            self.ctx.set_noise_buffer(None)
        try:
            self.ctx.render(self.mode, self.trav, (0, 0, w, h), k, spp, t["cur"].ptr, t["ids"].ptr)
        finally:
            if self.noise is not None:
                self.ctx.set_noise_buffer(self.noise.ptr)
            if self.counts is not None:
                self.ctx.set_adaptive(self.counts.ptr, **self.adaptive)
        new = 0 if t["latest"] is None else 1 - t["latest"]
        out = t["sets"][new]
        # (before update() moves the camera)
        self.ctx.denoise_guide(w, h, t["ids"].ptr, out["nz"].ptr, t["dz"].ptr, objects=self._guide_mask())
        hist = None
        if t["latest"] is not None:
            old = t["sets"][t["latest"]]
            hist = (old["color"].ptr, old["mom"].ptr, old["len"].ptr, old["nz"].ptr)
        scale = float(np.float32(k + spp) / np.float32(spp))
        self.ctx.temporal_accumulate(w, h, t["cur"].ptr, scale, out["nz"].ptr, t["uniform"], hist,
                                     (out["color"].ptr, out["mom"].ptr, out["len"].ptr), **t["params"])
        t["latest"] = new
        t["uniform"] = F.Uniform.from_buffer_copy(self.uniform)
        t["k"] = k + spp
        self.update()

    def temporal_current(self):
        """(accumulation float32 [H, W, 4], ids uint32 [H, W], uniform) of the most recent
        temporal_step's own render, for tests and tools."""
        t = self._temporal_or_raise(stepped=True)
        return (t["cur"].to_numpy(np.float32, (self.height, self.width, 4)),
                t["ids"].to_numpy(np.uint32, (self.height, self.width)), t["uniform"])

    def temporal_history(self):
        """(colour float32 [H, W, 4], moments float32 [H, W, 2], length uint32 [H, W]) of the latest frame."""
        t = self._temporal_or_raise(stepped=True)
        s = t["sets"][t["latest"]]
        return (s["color"].to_numpy(np.float32, (self.height, self.width, 4)),
                s["mom"].to_numpy(np.float32, (self.height, self.width, 2)),
                s["len"].to_numpy(np.uint32, (self.height, self.width)))

    def _temporal_check(self, levels, sigma_l, sigma_z):
        """(no device: the checks come before any allocation)"""
        self._temporal_or_raise(stepped=True)
        if not 1 <= int(levels) <= 5:
            raise ValueError("temporal_frame: levels must be in 1..5")
        if not (float(sigma_l) > 0.0 and float(sigma_z) > 0.0):
            raise ValueError("temporal_frame: the sigmas must be > 0")

    def _temporal_filter_into(self, out, levels, sigma_l, sigma_z):
        t = self.temporal
        s = t["sets"][t["latest"]]
        var = self.ctx.alloc(self.width * self.height * 4)
        try:
            self.ctx.temporal_variance(self.width, self.height, s["mom"].ptr, s["len"].ptr, s["nz"].ptr, t["dz"].ptr,
                                       var.ptr, min_len=t["min_len"], normal_min=t["params"]["normal_min"],
                                       plane_tol=t["params"]["plane_tol"])
            self.ctx.denoise_filter(self.width, self.height, s["color"].ptr, var.ptr, s["nz"].ptr, t["dz"].ptr, out.ptr,
                                    None, levels=levels, sigma_l=sigma_l, sigma_z=sigma_z)
            self.ctx.synchronize()
        finally:
            var.free()

    def temporal_frame(self, levels=5, sigma_l=4.0, sigma_z=1.0):
        """The latest integrated frame through rt_temporal_variance and rt_denoise_filter:
        float32 [H, W, 4], alpha 1."""
        self._temporal_check(levels, sigma_l, sigma_z)
        return self._filtered_frame(lambda out: self._temporal_filter_into(out, levels, sigma_l, sigma_z), rgba8=False)

    def temporal_rgba8(self, levels=5, sigma_l=4.0, sigma_z=1.0):
        """temporal_frame() as the sRGB surface would hold it: uint8 [H, W, 4] (rt_frame_rgba8_mode)."""
        self._temporal_check(levels, sigma_l, sigma_z)
        return self._filtered_frame(lambda out: self._temporal_filter_into(out, levels, sigma_l, sigma_z), rgba8=True)

    def frame(self):
        """Linear accumulation [H, W, 4] float32 (the RenderDestination texture)."""
        return self.accum.to_numpy(np.float32, (self.height, self.width, 4))

    def hit_ids(self):
        return self.ids.to_numpy(np.uint32, (self.height, self.width))

    def frame_rgba8(self):
        """The displayed frame as the sRGB surface holds it: uint8 [H, W, 4]
        (rt_frame_rgba8_mode, on the device: W1E2 and W1E3 without the pow)."""
        npx = self.width * self.height
        out = self.ctx.alloc(npx * 4)
        self.ctx.frame_rgba8(self.accum.ptr, npx, out.ptr, mode=self.mode)
        img = out.to_numpy(np.uint8, (self.height, self.width, 4))
        out.free()
        return img

    def save_png(self, path):
        """Write the displayed frame (PIL)."""
        from PIL import Image
        Image.fromarray(self.frame_rgba8(), "RGBA").save(path)

    @staticmethod
    def display(accum, mode=None):
        """fs_main's frame output: saturate(pow(accum, 1.5)) (w7e3.wgsl:265); for
        mode W1E2 or W1E3, whose shaders return the colour as it is, saturate(accum)."""
        x = np.maximum(accum[..., :3], 0)
        return np.clip(x if mode in F.LINEAR_DISPLAY_MODES else np.power(x, 1.5), 0, 1)
