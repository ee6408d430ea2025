// rt_scene.cpp -- the scene behind the C ABI (include/rt.h): storage-buffer uploads
// (replaces src/bindings/*.rs create_buffer_init) with the MI355X data layout repack,
// the device builders, downloads, uniforms, environment and textures, and the scene as
// the kernels read it (dev_scene).
#include "rt_ctx.h"

namespace {

// The traversal layout of the context's BSP (reference arrays already in
// bsp.ref_tree / bsp.ref_planes / bsp.ids, mesh in pos / idx): content boxes,
// 96-B treelets and the 48-B records (rt_layout.hip launch_bsp_repack), and
// the scale of the content boxes' margins: the largest coordinate magnitude of
// the BSP's root box (bsp_box_miss in rt_walk_bsp.h adds the ray origin's).
int repack_bsp(rt_ctx* c, uint32_t nnodes, uint32_t nids, size_t rec_off, size_t total, const float aabb[8])
{
    SceneState& s = c->scene;
    on_new_bsp(c);
    HIPCHK(c, s.bsp.nodes.alloc(total));
    DevBuf boxes;
    HIPCHK(c, boxes.alloc((size_t)nnodes * 64));
    HIPCHK(c, s.bsp.tm.alloc((size_t)std::max<uint32_t>(nids, 1u) * 8));
    if (rtk::launch_bsp_repack(s.bsp.ref_tree.as<uint32_t>(), s.bsp.ref_planes.as<float>(), nnodes, (uint32_t)rec_off,
                               s.bsp.nodes.p, s.pos.as<float4>(), s.idx.as<uint4>(), s.bsp.ids.as<uint32_t>(), nids,
                               0.0f, boxes.p, s.bsp.tm.as<uint2>(), c->stream))
        return fail(c, RT_E_DEVICE, "BSP repack launch failed");
    if (!s.bsp.plane_flag.p) HIPCHK(c, s.bsp.plane_flag.alloc(4));
    if (rtk::launch_plane_range(s.bsp.ref_tree.as<uint32_t>(), s.bsp.ref_planes.as<float>(), nnodes,
                                s.bsp.plane_flag.as<uint32_t>(), c->stream))
        return fail(c, RT_E_DEVICE, "BSP plane range launch failed");
    uint32_t pflag = 1;
    if (int r = read_back(c, &pflag, s.bsp.plane_flag.p, 4)) return r;
    s.bsp.div_checked = pflag != 0u;
    float scale = 0.0f;
    for (int k : {0, 1, 2, 4, 5, 6})
        if (std::isfinite(aabb[k])) scale = std::max(scale, std::fabs(aabb[k]));
    s.bsp.scale = scale;
    return RT_OK;
}

// Install a BSP of nnodes nodes and nids triangle slots on the context (rt_upload_bsp,
// rt_build_bsp_device).  One allocation [treelets | records], read through one buffer
// resource with 32-bit offsets (DESIGN.md "Data layout in HBM"), laid out on the
// device by launch_bsp_repack from the reference arrays, which place() puts into
// bsp.ref_tree / bsp.ref_planes / bsp.ids once the size is known to fit:
//  * treelet of node M (1-based heap index), 96 B at 96*M: M's content box,
//    the 8-B nodes {M | 2M, 2M+1 | 4M, 4M+1 | 4M+2, 4M+3} and the certified
//    culling's 16 B of subtree data -- everything a 3-level walk from M reads
//    (the nodes' encoding: rt_internal.h DevScene);
//  * record k (treeIds slot k): 48 B {v0, e0, e1, n} at rec_off + 48*k.
// who, detail: the caller's wording of the 4 GiB refusal.
template <class Place>
int install_bsp(rt_ctx* c, uint32_t nnodes, uint32_t nids, uint32_t max_depth, const float aabb8[8], const char* who,
                const char* detail, Place&& place)
{
    SceneState& s = c->scene;
    const size_t slots = (size_t)nnodes + 1;
    const size_t rec_off = (slots * rtk::BSP_TREELET_BYTES + 255) & ~(size_t)255;
    const size_t total = rec_off + (size_t)nids * 48;
    if (total >= ((size_t)1 << 32))
        return fail(c, RT_E_UNSUPPORTED, std::string(who) + ": BSP treelets + records must stay below 4 GiB" + detail);
    if (int r = place()) return r;
    if (int r = repack_bsp(c, nnodes, nids, rec_off, total, aabb8)) return r;
    s.bsp.rec_off = (uint32_t)rec_off;
    memcpy(s.bsp.aabb8, aabb8, sizeof s.bsp.aabb8);
    s.bsp.nnodes = nnodes;
    s.bsp.nids = nids;
    s.bsp.depth = max_depth;
    for (int k = 0; k < 3; k++) {
        s.aabb[k] = aabb8[k];
        s.aabb[k + 3] = aabb8[k + 4];
    }
    s.has_bsp = true;
    return RT_OK;
}

// Install a BVH of nnodes nodes and nids triangle slots on the context (rt_upload_bvh,
// rt_build_bvh_device).  One allocation [32-B node records | 48-B triangle records], read
// through one buffer resource with 32-bit offsets, laid out on the device by
// launch_bvh_repack from the reference arrays, which place() puts into bvh.ref / bvh.ids
// once the size is known to fit.  who: the caller's name in the messages.
template <class Place>
int install_bvh(rt_ctx* c, uint32_t nnodes, uint32_t nids, const char* who, Place&& place)
{
    SceneState& s = c->scene;
    const size_t rec_off = ((size_t)nnodes * 32 + 255) & ~(size_t)255;
    const size_t total = rec_off + (size_t)nids * 48;
    if (total >= ((size_t)1 << 32))
        return fail(c, RT_E_UNSUPPORTED, std::string(who) + ": BVH nodes + records must stay below 4 GiB");
    HIPCHK(c, s.bvh.nodes.alloc(total));
    if (int r = place()) return r;
    if (rtk::launch_bvh_repack(s.bvh.ref.as<rt_gpu_node>(), nnodes, (uint32_t)rec_off, s.bvh.nodes.p, s.pos.as<float4>(),
                               s.idx.as<uint4>(), s.bvh.ids.as<uint32_t>(), nids, c->stream))
        return fail(c, RT_E_DEVICE, std::string(who) + ": repack launch failed");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.bvh.rec_off = (uint32_t)rec_off;
    s.bvh.nnodes = nnodes;
    s.bvh.nids = nids;
    s.has_bvh = true;
    return RT_OK;
}

}  // namespace

// The camera terms of the treelets for the uniforms' eye (certified culling,
// rt_layout.hip launch_bsp_camera): recomputed when the eye moves.
int ensure_hcam(rt_ctx* c)
{
    SceneState& s = c->scene;
    CullState& k = c->cull;
    if (!s.has_bsp || !c->has_u || !cull_certified(c)) return RT_OK;
    const float* e = c->u.camera_pos;
    if (k.cam_valid && memcmp(e, k.cam_eye, sizeof k.cam_eye) == 0) return RT_OK;
    if (!(std::isfinite(e[0]) && std::isfinite(e[1]) && std::isfinite(e[2]))) return RT_OK;
    HIPCHK(c, k.cam_scratch.ensure((size_t)s.bsp.nnodes * 24));
    HIPCHK(c, k.sil.ensure(((size_t)s.bsp.nnodes + 1) * 16));
    HIPCHK(c, hipMemsetAsync(k.sil.p, 0, 16, c->stream));   // (slot 0: no node)
    if (rtk::launch_bsp_camera(s.bsp.ref_tree.as<uint32_t>(), s.bsp.nnodes, s.pos.as<float4>(), s.idx.as<uint4>(),
                               s.bsp.ids.as<uint32_t>(), s.bsp.nids, e, s.bsp.nodes.p, k.sil.as<uint32_t>(),
                               k.cam_scratch.p, c->stream))
        return fail(c, RT_E_DEVICE, "BSP camera terms: launch failed");
    memcpy(k.cam_eye, e, sizeof k.cam_eye);
    k.cam_valid = true;
    return RT_OK;
}

// The W5 modes' flat record array (rt_internal.h SweepScene): record i is triangle i of
// the index buffer -- the BSP repack is in treeIds order and cannot serve -- written by
// the record kernel in identity order (rt_layout.hip launch_tri_records) at the first W5
// render after an upload, zero-padded to a whole block of the sweep.
int ensure_sweep(rt_ctx* c)
{
    SceneState& s = c->scene;
    if (s.has_sweep) return RT_OK;
    const size_t padded = ((size_t)s.ntris + rtk::SWEEP_PAD_RECS) / rtk::SWEEP_PAD_RECS * rtk::SWEEP_PAD_RECS;
    HIPCHK(c, s.sweep_recs.alloc(padded * 48));
    HIPCHK(c, hipMemsetAsync(s.sweep_recs.as<uint8_t>() + (size_t)s.ntris * 48, 0, (padded - s.ntris) * 48, c->stream));
    if (rtk::launch_tri_records(s.pos.as<float4>(), s.idx.as<uint4>(), nullptr, s.ntris, s.sweep_recs.as<float4>(), nullptr,
                                c->stream))
        return fail(c, RT_E_DEVICE, "W5 records: launch failed");
    s.has_sweep = true;
    return RT_OK;
}

// The device-resident scene as the kernels read it (rt_internal.h DevScene).
rtk::DevScene dev_scene(const rt_ctx* c)
{
    const SceneState& s = c->scene;
    rtk::DevScene S;
    memset(&S, 0, sizeof S);
    for (int k = 0; k < 3; k++) S.cam_eye[k] = c->cull.cam_valid ? c->cull.cam_eye[k] : NAN;
    S.pos = s.pos.as<float4>();
    S.nrm = s.nrm.as<float4>();
    S.tri_idx = s.idx.as<uint4>();
    S.mats = s.mats.as<rt_material>();
    S.lights = s.lights.as<uint32_t>();
    S.nverts = s.nverts;
    S.ntris = s.ntris;
    S.nmats = s.nmats;
    S.nlights = s.nlights;
    S.bsp_nodes = s.bsp.nodes.as<uint2>();
    S.bsp_recs = reinterpret_cast<const float4*>(s.bsp.nodes.as<uint8_t>() + s.bsp.rec_off);
    S.bsp_bytes = (uint32_t)s.bsp.nodes.n;
    S.bsp_rec_off = s.bsp.rec_off;
    S.bsp_ids = s.bsp.ids.as<uint32_t>();
    S.bsp_tm = s.bsp.tm.as<uint2>();
    S.bsp_sil = c->cull.sil.as<uint4>();
    S.bsp_cull_mode = cull_in_use(c);
    S.bsp_div_checked = s.bsp.div_checked;
    S.bsp_depth = s.bsp.depth;
    memcpy(S.aabb, s.aabb, sizeof S.aabb);
    S.bvh_base = s.bvh.nodes.as<uint8_t>();
    S.bvh_bytes = (uint32_t)s.bvh.nodes.n;
    S.bvh_rec_off = s.bvh.rec_off;
    S.bvh_ids = s.bvh.ids.as<uint32_t>();
    S.bvh_nnodes = s.bvh.nnodes;
    // the culling margin as data (rt_internal.h DevScene, rt_walk_bsp.h bsp_box_miss)
    S.bsp_cull_gap = c->bsp_cull != RT_BSP_CULL_OFF ? 0x1p-18f : INFINITY;
    S.bsp_cull_emax = c->bsp_cull != RT_BSP_CULL_OFF ? FLT_MAX : INFINITY;
    // off: the fast formula's constants (k1 = 0 picks k_path's fast-margin
    // instantiation, launch_path); the +inf gap culls nothing either way
    if (!cull_certified(c)) {
        S.cull_k1 = 0.0f;
        S.cull_k3 = 0.0f;
        S.cull_ko = 0x1p-10f;
        S.bsp_margin = std::ldexp(s.bsp.scale, -10);
    } else {
        S.cull_k1 = 36.0f * 0x1p-24f;
        S.cull_k3 = 2.0f * 0x1p-24f;
        S.cull_ko = 0x1p-19f;
        S.bsp_margin = std::ldexp(s.bsp.scale, -19);
    }
    return S;
}

extern "C" {

int rt_upload_mesh(rt_ctx* c, const float* pos_vec4, const float* nrm_vec4, uint32_t nverts,
                   const uint32_t* idx_vec4u, uint32_t ntris, const rt_material* mats, uint32_t nmats,
                   const uint32_t* light_idx, uint32_t nlight)
{
    if (!c) return RT_E_INVALID;
    if ((!pos_vec4 && nverts) || (!idx_vec4u && ntris) || !mats || nmats == 0)
        return fail(c, RT_E_INVALID, "rt_upload_mesh: missing arrays (need >= 1 material)");
    for (size_t t = 0; t < ntris; t++)
        for (int k = 0; k < 3; k++)
            if (idx_vec4u[t * 4 + k] >= nverts) return fail(c, RT_E_INVALID, "rt_upload_mesh: vertex index out of range");
    std::vector<uint32_t> lights;
    if (light_idx) {
        if (nlight == 0 || light_idx[0] != 0xFFFFFFFFu)
            return fail(c, RT_E_INVALID, "rt_upload_mesh: light list must start with the UINT32_MAX sentinel");
        lights.assign(light_idx, light_idx + nlight);
        for (uint32_t i = 1; i < nlight; i++)
            if (lights[i] >= ntris) return fail(c, RT_E_INVALID, "rt_upload_mesh: light index out of range");
    } else {
        std::vector<uint32_t> ix(idx_vec4u, idx_vec4u + (size_t)ntris * 4);
        std::vector<rt_material> mv(mats, mats + nmats);
        lights = rthost::light_list(ix, mv);
    }
    if (int r = set_dev(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    SceneState& s = c->scene;
    s.has_mesh = s.has_bsp = s.has_bvh = s.has_sweep = false;
    std::vector<float> nrm;
    if (nrm_vec4) nrm.assign(nrm_vec4, nrm_vec4 + (size_t)nverts * 4);
    else nrm.assign((size_t)nverts * 4, 0.0f);
    int r;
    if ((r = upload(c, s.pos, pos_vec4, (size_t)nverts * 16))) return r;
    if ((r = upload(c, s.nrm, nrm.data(), nrm.size() * 4))) return r;
    if ((r = upload(c, s.idx, idx_vec4u, (size_t)ntris * 16))) return r;
    if ((r = upload(c, s.mats, mats, (size_t)nmats * sizeof(rt_material)))) return r;
    if ((r = upload(c, s.lights, lights.data(), lights.size() * 4))) return r;
    s.nverts = nverts;
    s.ntris = ntris;
    s.nmats = nmats;
    s.nlights = (uint32_t)lights.size();
    s.has_mesh = true;
    // (as rt_empty_mask_host: the finite coordinates' largest magnitude)
    s.mesh_scale = 0.0f;
    for (size_t v = 0; v < nverts; v++)
        for (int a = 0; a < 3; a++) {
            const float x = pos_vec4[4 * v + a];
            if (x - x == 0.0f) s.mesh_scale = std::max(s.mesh_scale, x < 0 ? -x : x);
        }
    on_new_mesh(c);
    return RT_OK;
}

int rt_upload_bsp(rt_ctx* c, const float aabb[8], const uint32_t* tree, const float* planes, uint32_t nnodes,
                  const uint32_t* ids, uint32_t nids, uint32_t max_depth)
{
    if (!c) return RT_E_INVALID;
    SceneState& s = c->scene;
    if (!s.has_mesh) return fail(c, RT_E_NOT_READY, "rt_upload_bsp: upload the mesh first");
    if (!aabb || !tree || !planes || (!ids && nids)) return fail(c, RT_E_INVALID, "rt_upload_bsp: null array");
    if (max_depth == 0 || max_depth >= 32 || (uint64_t)nnodes != ((uint64_t)1 << (max_depth + 1)) - 1)
        return fail(c, RT_E_INVALID, "rt_upload_bsp: nnodes must be 2^(max_depth+1)-1, max_depth in [1,31]");
    for (uint32_t k = 0; k < nids; k++)
        if (ids[k] >= s.ntris) return fail(c, RT_E_INVALID, "rt_upload_bsp: triangle id out of range");
    // validate the reachable tree (implicit children, leaves inside ids)
    std::vector<uint32_t> stack{0};
    while (!stack.empty()) {
        const uint32_t i = stack.back();
        stack.pop_back();
        const uint32_t* n = tree + 4 * (size_t)i;
        if ((n[0] & 3u) == 3u) {
            if ((uint64_t)n[1] + (n[0] >> 2) > nids)
                return fail(c, RT_E_INVALID, "rt_upload_bsp: leaf range outside treeIds");
            if ((n[0] >> 2) >= (1u << 24))
                return fail(c, RT_E_UNSUPPORTED, "rt_upload_bsp: leaf with 2^24 or more triangles");
            continue;
        }
        const uint64_t l = 2ull * i + 1, rgt = 2ull * i + 2;
        if (rgt >= nnodes || n[2] != l || n[3] != rgt)
            return fail(c, RT_E_INVALID, "rt_upload_bsp: interior node children are not 2i+1, 2i+2 inside the array");
        stack.push_back((uint32_t)l);
        stack.push_back((uint32_t)rgt);
    }
    if (int r = set_dev(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.has_bsp = false;
    return install_bsp(c, nnodes, nids, max_depth, aabb, "rt_upload_bsp",
                       " (96-B treelets: max_depth 24 takes 3.2 GB, leaving room for ~22M records)", [&] {
                           if (int r = upload(c, s.bsp.ref_tree, tree, (size_t)nnodes * 16)) return r;
                           if (int r = upload(c, s.bsp.ref_planes, planes, (size_t)nnodes * 4)) return r;
                           return upload(c, s.bsp.ids, ids, (size_t)nids * 4);
                       });
}

int rt_upload_bvh(rt_ctx* c, const rt_gpu_node* nodes, uint32_t nnodes, const uint32_t* tri_ids, uint32_t nids)
{
    if (!c) return RT_E_INVALID;
    SceneState& s = c->scene;
    if (!s.has_mesh) return fail(c, RT_E_NOT_READY, "rt_upload_bvh: upload the mesh first");
    if (!nodes || nnodes == 0 || (!tri_ids && nids)) return fail(c, RT_E_INVALID, "rt_upload_bvh: null array");
    for (uint32_t k = 0; k < nids; k++)
        if (tri_ids[k] >= s.ntris) return fail(c, RT_E_INVALID, "rt_upload_bvh: triangle id out of range");
    // validate nodes reachable from the root (bvh.wgsl:168-179 walk)
    std::vector<uint8_t> seen(nnodes, 0);
    std::vector<uint32_t> stack{0};
    while (!stack.empty()) {
        const uint32_t i = stack.back();
        stack.pop_back();
        if (seen[i]) continue;
        seen[i] = 1;
        const rt_gpu_node& n = nodes[i];
        if (n.n_prims > 0) {
            if ((uint64_t)n.offset_ptr + n.n_prims > nids) return fail(c, RT_E_INVALID, "rt_upload_bvh: leaf range");
        } else {
            if ((uint64_t)i + 1 >= nnodes || n.offset_ptr >= nnodes)
                return fail(c, RT_E_INVALID, "rt_upload_bvh: child index out of range");
            stack.push_back(i + 1);
            stack.push_back(n.offset_ptr);
        }
    }
    if (int r = set_dev(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.has_bvh = false;
    return install_bvh(c, nnodes, nids, "rt_upload_bvh", [&] {
        if (int r = upload(c, s.bvh.ids, tri_ids, (size_t)nids * 4)) return r;
        return upload(c, s.bvh.ref, nodes, (size_t)nnodes * sizeof(rt_gpu_node));
    });
}

int rt_build_bvh_device(rt_ctx* c, uint32_t max_prims, rt_bvh_build_times* times)
{
    if (!c) return RT_E_INVALID;
    SceneState& s = c->scene;
    if (!s.has_mesh) return fail(c, RT_E_NOT_READY, "rt_build_bvh_device: upload the mesh first");
    if (max_prims == 0) return fail(c, RT_E_INVALID, "rt_build_bvh_device: max_prims must be >= 1");
    if (int r = set_dev(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.has_bvh = false;
    rtk::BvhDeviceOut o;
    std::string err;
    const int r = rtk::build_bvh_device(s.pos.as<float4>(), s.idx.as<uint4>(), s.ntris, max_prims, c->num_cus,
                                        c->stream, o, times, err);
    DevBuf nodes_ref, ids;   // own the outputs from here on
    if (o.nodes) nodes_ref.adopt(o.nodes, (size_t)o.nnodes * sizeof(rt_gpu_node));
    if (o.ids) ids.adopt(o.ids, (size_t)o.nids * 4);
    if (r) return fail(c, r, err);
    return install_bvh(c, o.nnodes, o.nids, "rt_build_bvh_device", [&] {
        s.bvh.ref.adopt(nodes_ref.p, nodes_ref.n);
        nodes_ref.p = nullptr;
        s.bvh.ids.adopt(ids.p, ids.n);
        ids.p = nullptr;
        return (int)RT_OK;
    });
}

int rt_build_bsp_device(rt_ctx* c, uint32_t max_depth, uint32_t max_leaf, rt_bsp_build_times* times)
{
    if (!c) return RT_E_INVALID;
    SceneState& s = c->scene;
    if (!s.has_mesh) return fail(c, RT_E_NOT_READY, "rt_build_bsp_device: upload the mesh first");
    if (int r = set_dev(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.has_bsp = false;
    rtk::BspDeviceOut o;
    std::string err;
    const int r = rtk::build_bsp_device(s.pos.as<float4>(), s.idx.as<uint4>(), s.ntris, max_depth, max_leaf,
                                        c->num_cus, c->stream, o, times, err);
    DevBuf tree, planes, ids;   // own the outputs from here on
    if (o.tree) tree.adopt(o.tree, (size_t)o.nnodes * 16);
    if (o.planes) planes.adopt(o.planes, (size_t)o.nnodes * 4);
    if (o.ids) ids.adopt(o.ids, std::max<size_t>(16, (size_t)o.nids * 4));
    if (r) return fail(c, r, err);
    return install_bsp(c, o.nnodes, o.nids, max_depth, o.aabb, "rt_build_bsp_device", "", [&] {
        s.bsp.ref_tree.adopt(tree.p, tree.n);
        tree.p = nullptr;
        s.bsp.ref_planes.adopt(planes.p, planes.n);
        planes.p = nullptr;
        s.bsp.ids.adopt(ids.p, ids.n);
        ids.p = nullptr;
        return (int)RT_OK;
    });
}

int rt_download_bsp(rt_ctx* c, uint32_t* tree, float* planes, uint32_t cap_nodes, uint32_t* ids, uint32_t cap_ids,
                    float aabb[8], uint32_t* nnodes, uint32_t* nids)
{
    if (!c) return RT_E_INVALID;
    const SceneState::Bsp& b = c->scene.bsp;
    if (!c->scene.has_bsp) return fail(c, RT_E_NOT_READY, "rt_download_bsp: no BSP on the context");
    if (nnodes) *nnodes = b.nnodes;
    if (nids) *nids = b.nids;
    if (aabb) memcpy(aabb, b.aabb8, sizeof b.aabb8);
    if (int r = set_dev(c)) return r;
    if ((tree || planes) && cap_nodes < b.nnodes) return fail(c, RT_E_INVALID, "rt_download_bsp: arrays too small");
    if (ids && cap_ids < b.nids) return fail(c, RT_E_INVALID, "rt_download_bsp: id array too small");
    if (tree) HIPCHK(c, hipMemcpyAsync(tree, b.ref_tree.p, (size_t)b.nnodes * 16, hipMemcpyDeviceToHost, c->stream));
    if (planes)
        HIPCHK(c, hipMemcpyAsync(planes, b.ref_planes.p, (size_t)b.nnodes * 4, hipMemcpyDeviceToHost, c->stream));
    if (ids && b.nids) HIPCHK(c, hipMemcpyAsync(ids, b.ids.p, (size_t)b.nids * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

int rt_download_bsp_treelets(rt_ctx* c, void* dst, uint64_t cap_bytes, uint64_t* bytes)
{
    if (!c) return RT_E_INVALID;
    if (!c->scene.has_bsp) return fail(c, RT_E_NOT_READY, "rt_download_bsp_treelets: no BSP on the context");
    const uint64_t nt = ((uint64_t)c->scene.bsp.nnodes + 1) * rtk::BSP_TREELET_BYTES;
    const uint64_t ns = ((uint64_t)c->scene.bsp.nnodes + 1) * 16;
    const uint64_t n = nt + ns;
    if (bytes) *bytes = n;
    if (!dst) return RT_OK;
    if (cap_bytes < n) return fail(c, RT_E_INVALID, "rt_download_bsp_treelets: buffer too small");
    if (int r = set_dev(c)) return r;   // (first: ensure_hcam may launch the camera-term kernels)
    if (int r = ensure_hcam(c)) return r;
    HIPCHK(c, hipMemcpyAsync(dst, c->scene.bsp.nodes.p, nt, hipMemcpyDeviceToHost, c->stream));
    // the silhouette section only when it was made for this BSP and the uniforms' eye
    // (ensure_hcam leaves it alone in the uncertified modes)
    const bool sil_now = c->cull.cam_valid && cull_certified(c) && c->has_u &&
                         memcmp(c->u.camera_pos, c->cull.cam_eye, sizeof c->cull.cam_eye) == 0;
    if (sil_now && c->cull.sil.n >= ns) HIPCHK(c, hipMemcpyAsync(static_cast<uint8_t*>(dst) + nt, c->cull.sil.p, ns,
                                                     hipMemcpyDeviceToHost, c->stream));
    else memset(static_cast<uint8_t*>(dst) + nt, 0, ns);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

int rt_download_bvh(rt_ctx* c, rt_gpu_node* nodes, uint32_t cap_nodes, uint32_t* tri_ids, uint32_t cap_ids,
                    uint32_t* nnodes, uint32_t* nids)
{
    if (!c) return RT_E_INVALID;
    const SceneState::Bvh& b = c->scene.bvh;
    if (!c->scene.has_bvh) return fail(c, RT_E_NOT_READY, "rt_download_bvh: no BVH on the context");
    if (nnodes) *nnodes = b.nnodes;
    if (nids) *nids = b.nids;
    if (int r = set_dev(c)) return r;
    if (nodes) {
        if (cap_nodes < b.nnodes) return fail(c, RT_E_INVALID, "rt_download_bvh: node array too small");
        HIPCHK(c, hipMemcpyAsync(nodes, b.ref.p, (size_t)b.nnodes * sizeof(rt_gpu_node), hipMemcpyDeviceToHost,
                                 c->stream));
    }
    if (tri_ids) {
        if (cap_ids < b.nids) return fail(c, RT_E_INVALID, "rt_download_bvh: id array too small");
        HIPCHK(c, hipMemcpyAsync(tri_ids, b.ids.p, (size_t)b.nids * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

int rt_set_uniforms(rt_ctx* c, const rt_uniform* u, const float* jitter)
{
    if (!c || !u) return RT_E_INVALID;
    if (u->resolution[0] == 0 || u->resolution[1] == 0) return fail(c, RT_E_INVALID, "rt_set_uniforms: zero resolution");
    // k_path packs a lane's pixel as x | y << 16
    if (u->resolution[0] > 65535u || u->resolution[1] > 65535u)
        return fail(c, RT_E_INVALID, "rt_set_uniforms: resolution above 65535");
    if (u->subdivision_level == 0 || u->subdivision_level > 10)
        return fail(c, RT_E_INVALID, "rt_set_uniforms: subdivision_level must be in [1,10] (uniform.rs:36)");
    if (!jitter && u->subdivision_level != 1)
        return fail(c, RT_E_INVALID, "rt_set_uniforms: jitter table required when subdivision_level > 1");
    if (int r = set_dev(c)) return r;
    c->u = *u;
    c->has_u = true;
    c->has_jitter = false;
    if (jitter) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const size_t bytes = (size_t)u->subdivision_level * u->subdivision_level * 2 * sizeof(float);
        if (int r = upload(c, c->jitter, jitter, bytes)) return r;
        c->has_jitter = true;
    }
    return RT_OK;
}

int rt_set_environment(rt_ctx* c, const float rgb[3])
{
    if (!c || !rgb) return RT_E_INVALID;
    memcpy(c->env, rgb, sizeof c->env);
    return RT_OK;
}

// an RGBA8 texture of width x height texels into buf (its size into *w, *h)
static int set_rgba8(rt_ctx* c, const char* who, DevBuf& buf, uint32_t* w, uint32_t* h, const uint8_t* rgba8,
                     uint32_t width, uint32_t height)
{
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 31))
        return fail(c, RT_E_INVALID, std::string(who) + ": bad texture size");
    if (int r = set_dev(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int r = upload(c, buf, rgba8, (size_t)width * height * 4)) return r;
    *w = width;
    *h = height;
    return RT_OK;
}

int rt_set_environment_map(rt_ctx* c, const uint8_t* rgba8, uint32_t width, uint32_t height)
{
    if (!c) return RT_E_INVALID;
    if (rgba8) return set_rgba8(c, "rt_set_environment_map", c->env_tex, &c->env_w, &c->env_h, rgba8, width, height);
    c->env_tex.reset();
    c->env_w = c->env_h = 0;
    return RT_OK;
}

int rt_set_texture(rt_ctx* c, const uint8_t* rgba8, uint32_t width, uint32_t height)
{
    if (!c) return RT_E_INVALID;
    if (rgba8) return set_rgba8(c, "rt_set_texture", c->tex0, &c->tex0_w, &c->tex0_h, rgba8, width, height);
    if (c->tex0.p) {   // a render that reads it may still be in flight
        if (int r = set_dev(c)) return r;
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->tex0.reset();
    c->tex0_w = c->tex0_h = 0;
    return RT_OK;
}

int rt_upload_mesh_host(rt_ctx* c, const rt_mesh_host* m)
{
    if (!c || !m) return RT_E_INVALID;
    return rt_upload_mesh(c, m->pos.data(), m->nrm.data(), m->nverts(), m->idx.data(), m->ntris(), m->mats.data(),
                          (uint32_t)m->mats.size(), m->lights.data(), (uint32_t)m->lights.size());
}

int rt_upload_bsp_host(rt_ctx* c, const rt_bsp_host* b)
{
    if (!c || !b) return RT_E_INVALID;
    return rt_upload_bsp(c, b->aabb, b->tree.data(), b->planes.data(), (uint32_t)b->planes.size(), b->ids.data(),
                         (uint32_t)b->ids.size(), b->max_depth);
}

int rt_upload_bvh_host(rt_ctx* c, const rt_bvh_host* b)
{
    if (!c || !b) return RT_E_INVALID;
    return rt_upload_bvh(c, b->nodes.data(), (uint32_t)b->nodes.size(), b->tri_ids.data(), (uint32_t)b->tri_ids.size());
}

}  // extern "C"
