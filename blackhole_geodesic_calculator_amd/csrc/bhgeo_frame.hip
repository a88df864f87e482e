// bhgeo_frame.hip -- the library-owned FRAME of libbhgeo.so (bhg_frame_* in include/bhgeo.h): jitter stream -> camera
// rays -> geodesics -> shaded, sample-averaged float RGBA pixels in frame order, on one or several GPUs of ONE process,
// with no PyTorch (or Python) anywhere near it.
//
// What it replaces: the whole body of the reference's frame loop, raytracer/RelativisticRenderEngine.py:172-267
// (ray_trace: pinhole + jitter :224-230, the per-ray solve :232 -> :293-294, background_hit :366-378, the sample mean
// :242-250) as Blender calls it -- render() :50 -> render_scene() :152-168 on ONE render thread of ONE process; the
// author's commented-out mp.Pool (:210-216) marks where the parallelism has to live.  Here: one host thread drives one
// bhg_context per listed device; 32x32-pixel tiles are dealt to the devices (all samples of a pixel on one device), each
// device generates, traces and shades its shard into a slab, the slabs are gathered onto the first device -- RCCL in
// single-process mode (ncclCommInitAll, grouped ncclSend / ncclRecv over xGMI) when the devices are distinct, plain
// device-to-device copies when the list repeats a device or RCCL cannot be loaded -- put into frame order by one kernel
// and handed back as one array.
//
// Built on the public C ABI (bhg_create, bhg_trace*_device, bhg_shade*_device, bhg_assemble_frame_f32_device): the frame
// is a client of the same boundary every other caller uses; only the ray generation goes to the internal launcher, for
// its compact-jitter form (each device gets the draws of ITS pixels, not the whole frame's stream).
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "bhgeo_internal.h"
#include "mesh_bvh.h"
#include "prefix_clearance.h"
#include "tile_dealing.h"

namespace {

// No C++ exception leaves the library through the C ABI: the entry points that use standard containers (the jitter stream and
// the images are copied into vectors, the tile dealing sorts) are function-try-blocks that end here.
int host_exception()
{
    try {
        throw;
    } catch (const std::bad_alloc &) {
        return fail(BHG_E_NOMEM, "host allocation failed");
    } catch (const std::exception &e) {
        return fail(BHG_E_HIP, std::string("internal error: ") + e.what());
    } catch (...) {
        return fail(BHG_E_HIP, "internal error: unknown exception");
    }
}

// ---- RCCL, loaded at run time (libbhgeo.so itself links only the HIP runtime) ---------------------------------------
typedef void *nccl_comm_t;
struct Rccl {
    void *lib = nullptr;
    int (*CommInitAll)(nccl_comm_t *, int, const int *) = nullptr;
    int (*CommDestroy)(nccl_comm_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void *, size_t, int, int, nccl_comm_t, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, nccl_comm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool ok() const { return lib != nullptr; }
};
constexpr int NCCL_FLOAT32 = 7;   // ncclFloat32 (rccl.h)

Rccl load_rccl()
{
    Rccl r;
    // by SONAME first: a host process that already carries RCCL (PyTorch-ROCm bundles one) keeps ONE copy
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *h = nullptr;
    for (const char *n : names)
        if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h) return r;
    Rccl t;
    t.lib = h;
    t.CommInitAll = (decltype(t.CommInitAll))dlsym(h, "ncclCommInitAll");
    t.CommDestroy = (decltype(t.CommDestroy))dlsym(h, "ncclCommDestroy");
    t.GroupStart = (decltype(t.GroupStart))dlsym(h, "ncclGroupStart");
    t.GroupEnd = (decltype(t.GroupEnd))dlsym(h, "ncclGroupEnd");
    t.Send = (decltype(t.Send))dlsym(h, "ncclSend");
    t.Recv = (decltype(t.Recv))dlsym(h, "ncclRecv");
    t.GetErrorString = (decltype(t.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (t.CommInitAll && t.CommDestroy && t.GroupStart && t.GroupEnd && t.Send && t.Recv && t.GetErrorString) r = t;
    return r;
}

Rccl &rccl()
{
    static Rccl r = load_rccl();   // (a function-local static: initialised once, also when two threads create frames at once)
    return r;
}

int fail_nccl(int e, const char *what)
{
    return fail(BHG_E_HIP, std::string(what) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(e) : "RCCL error"));
}
#define NCCL_TRY(expr)                         \
    do {                                       \
        int _e = (expr);                       \
        if (_e != 0) return fail_nccl(_e, #expr); \
    } while (0)

struct DevBuf {   // a device allocation that remembers its device
    void *p = nullptr;
    size_t bytes = 0;
    int device = 0;
    int ensure(int dev, size_t need)
    {
        if (p && bytes >= need && dev == device) return BHG_OK;
        release();
        if (need == 0) return BHG_OK;
        HIP_TRY(hipSetDevice(dev));
        HIP_TRY(hipMalloc(&p, need));
        bytes = need;
        device = dev;
        return BHG_OK;
    }
    void release()
    {
        if (p) {
            (void)hipSetDevice(device);
            (void)hipFree(p);
        }
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T *as() const { return (T *)p; }
};

struct Shard {
    int device = 0;
    bhg_context *ctx = nullptr;
    hipStream_t stream = nullptr;   // the context's own
    std::vector<int64_t> pixels;    // flat ids y * W + x, tile after tile
    size_t P = 0, n = 0;
    DevBuf pixels_d, jitter_d, k0, end, dir, flags, steps, acc, obj, slab, sky, disk_tex;
    DevBuf start_h;                 // [n] doubles beside k0: the rays' initial steps, kept from render to render (BHG_START_STEPS)
    DevBuf start_rec;               // the rays' start-up records (BHG_START_PREFIX: 112 B per ray), written by the render that records
    bhg::PrefixOwner start_owner;   // ... their radius (0: none are held) and when to record them again, scene change by scene change
    bhg_prefix start_last = {nullptr, 0.0, BHG_PREFIX_NONE, BHG_PREFIX_NONE};   // what the last render asked for and was told
    DevBuf otex[BHG_MAX_SPHERES];   // the object textures (bhg_frame_set_object_textures), slot by slot
    // the mesh (bhg_frame_set_mesh): this device's copy, its material's arrays and images, the mesh trace's hit records
    bhg_mesh *mesh = nullptr;
    DevBuf m_rgb, m_uv, m_slot, m_img[BHG_MESH_TEXTURES_MAX], tri, bary;
    bool mesh_ready = false;        // mesh and the material buffers hold the frame's current mesh
    bool mesh_refit = false;        // ... but for the vertices (bhg_frame_refit_mesh): the next render refits (or rebuilds) the tree
    int32_t mesh_leaf = 0;          // leaf_size and normals of `mesh`: what a rebuild in place must find unchanged (section 23)
    bool mesh_normals = false;
    // the mesh's instances (bhg_frame_set_mesh_instances): this device's set over mesh, the colours, the trace's third record
    bhg_mesh_instances *inst = nullptr;
    int32_t inst_n = 0;
    int32_t inst_leaf = 0;          // the leaf_size of the tree inst lies under (0: a linear set)
    DevBuf inst_rgb, inst_id;
    bool inst_ready = false;        // inst holds the frame's current transforms, inst_rgb its colours
    hipEvent_t done = nullptr;
    bool rays_ready = false;
    bool start_ready = false;       // start_h holds the steps of the rays in k0, traced from start_origin with start_prm
    bhg_params start_prm = {};
    double start_origin[3] = {0, 0, 0};
    void drop_rays() { rays_ready = start_ready = false; }   // the rays in k0 are to be made anew: their steps go with them
    bool jitter_ready = false;      // jitter_d holds the draws of THIS pixel list (kept: a rotating camera regenerates the rays from it)
    bool scene_ready = false;
    bool otex_ready = false;        // otex holds the frame's current object textures
    bool dir_traced = false;
    nccl_comm_t comm = nullptr;
    // profiling: HIP event pairs around the trace call of every profiled render since the last bhg_frame_last_ms()
    std::vector<std::pair<hipEvent_t, hipEvent_t>> evs;
    size_t ev_used = 0;
};

}  // namespace

struct bhg_frame {
    bhg_camera cam;
    int32_t tile = 32;
    int32_t gather = BHG_FRAME_GATHER_COPY;   // the mode in use (never AUTO)
    std::vector<Shard> sh;
    std::vector<double> jitter;     // host copy of the caller's stream (empty: pixel centres)
    // scene (host copies; uploaded to every device on the next render)
    std::vector<float> sky, disk_tex;
    int32_t sky_w = 0, sky_h = 0, disk_w = 0, disk_h = 0;
    bhg_frame_scene scene;          // (its pointers are not used after bhg_frame_set_scene)
    bhg_redshift rs = {0u, 1, 4.0}; // bhg_frame_set_redshift; apply = 0: off (the shade calls of ABI 8)
    bool observer = false;          // bhg_frame_set_observer; false: the reference camera (the ray generation of ABI 9)
    bhg_observer obs = {{0.0, 0.0, 0.0}};
    double obs_key[6] = {};         // camera origin, r_s, spin, rhs_form the observer rays on the devices were made for
    bool textured = false;          // bhg_frame_set_object_textures; false: the object shading without textures
    bhg_object_textures ot = {};    // its rotations, modes and strengths (tex: not used, the images are otex)
    std::vector<float> otex[BHG_MAX_SPHERES];    // host copies of the object textures, empty = white
    bool thermal = false;           // bhg_frame_set_disk_thermal; false: the disk's colour of the scene
    bhg_disk_thermal th = {};
    bool moving = false;            // bhg_frame_set_object_motion; false: the object spheres at rest
    bhg_object_motion mo = {};
    int32_t otex_w[BHG_MAX_SPHERES] = {}, otex_h[BHG_MAX_SPHERES] = {};
    // bhg_frame_set_mesh: host copies of the mesh and its material (uploaded to every device on the next render)
    struct Mesh {
        std::vector<double> vertices, normals;      // normals empty: flat shading
        std::vector<int32_t> triangles;
        int32_t leaf_size = 4;
        double max_chord = 0.0;                     // 0: a quarter of the render's r_s
        std::vector<float> tri_rgb, tri_uv;         // empty: white / no textures
        std::vector<int32_t> tri_tex;               // empty: slot 0 for every triangle
        std::vector<float> img[BHG_MESH_TEXTURES_MAX];
        int32_t img_w[BHG_MESH_TEXTURES_MAX] = {}, img_h[BHG_MESH_TEXTURES_MAX] = {};
        int32_t n_tex = 0;
        double emission = 0.0;
        double rebuild_ratio = 0.0;                 // of the latest bhg_frame_refit_mesh
    };
    bool meshed = false;            // bhg_frame_set_mesh; false: no mesh, the plain render
    bool mesh_build_device = false; // bhg_frame_set_mesh_build: trees are built (and rebuilt in place) on the devices
    Mesh mesh;
    // bhg_frame_set_mesh_instances: host copies (empty: the mesh where its vertices put it)
    std::vector<double> inst;       // [n][12]
    int32_t inst_leaf = 0;          // bhg_frame_set_mesh_instance_tree: the leaf_size of the sets' trees (0: linear sets)
    std::vector<float> inst_rgb;    // [n][3], or empty
    // root (device of shard 0)
    DevBuf recv, perm, image;       // [n_dev * pmax][4] float, [H W] int64, [H W][4] float
    size_t pmax = 0;
    void *pin = nullptr;            // page-locked staging of the image for pageable callers
    size_t pin_bytes = 0;
    std::vector<double> tile_cost;  // measured attempted steps per tile of the last render (bhg_frame_rebalance)
    bool dealt_by_cost = false;
    double root_share = 1.0;        // part of an equal share the first device is dealt (bhg_frame_rebalance)
    bool rendered = false;
    bool profiling = false;
    bool peer_copy_always = false;  // BHG_FRAME_GATHER_COPY_PEERCALL: the gather's copies go through hipMemcpyPeerAsync also between
                                    // contexts of ONE device (the N-device call on a one-GPU box)
    std::vector<hipEvent_t> ev_root;   // around the root's gather + assembly (profiling)
    std::vector<hipEvent_t> ev_piece;  // the pieces of the image's way back to a pageable caller array
    hipEvent_t assembled = nullptr;    // the root has read the receive block of the last render (copies of the next wait for it)
    uint64_t renders = 0;
};

namespace {

// ---- tile dealing: tile_dealing.h (plain C++, also built with the host compiler under sanitizers) ------------------
using bhg::deal_tiles_into;

void deal_tiles(bhg_frame *f)
{
    const int W = f->cam.width, H = f->cam.height, T = f->tile, world = (int)f->sh.size();
    const int nt = ((W + T - 1) / T) * ((H + T - 1) / T);
    const bool by_cost = f->dealt_by_cost && (int)f->tile_cost.size() == nt;
    std::vector<std::vector<int64_t>> px;
    deal_tiles_into(W, H, T, world, by_cost ? f->tile_cost.data() : nullptr, world > 1, f->root_share, px);
    f->pmax = 0;
    for (size_t r = 0; r < f->sh.size(); r++) {
        Shard &s = f->sh[r];
        s.pixels.swap(px[r]);
        s.P = s.pixels.size();
        s.n = s.P * (size_t)f->cam.samples;
        s.drop_rays();
        s.jitter_ready = false;
        f->pmax = std::max(f->pmax, s.P);
    }
    // the devices' steps / flags arrays still hold the PREVIOUS pixel lists' rays (and may be smaller than the new shards):
    // nothing may read them by the new lists until the next render
    f->rendered = false;
}

// obs: nullptr, or the observer camera the rays are made for (checked by the caller)
int upload_shard_geometry(bhg_frame *f, Shard &s, const bhg::ObserverParams *obs)
{
    // pixel list, compact jitter [S][P][2] in list order, ray buffers
    const size_t S = (size_t)f->cam.samples, frame_px = (size_t)f->cam.width * (size_t)f->cam.height;
    HIP_TRY(hipSetDevice(s.device));
    BHG_TRY(s.pixels_d.ensure(s.device, s.P * sizeof(int64_t)));
    BHG_TRY(s.k0.ensure(s.device, s.n * 3 * sizeof(double)));
    BHG_TRY(s.flags.ensure(s.device, s.n));
    BHG_TRY(s.steps.ensure(s.device, s.n * sizeof(uint32_t)));
    BHG_TRY(s.acc.ensure(s.device, s.n * sizeof(uint32_t)));
    s.start_ready = false;   // (whoever asked for new rays has said so already; new rays never meet old steps)
    if (s.P == 0) {
        s.rays_ready = true;
        return BHG_OK;
    }
    HIP_TRY(hipMemcpyAsync(s.pixels_d.p, s.pixels.data(), s.P * sizeof(int64_t), hipMemcpyHostToDevice, s.stream));
    std::vector<double> jc;
    if (!f->jitter.empty() && !s.jitter_ready) {
        jc.resize(2 * S * s.P);
        for (size_t sm = 0; sm < S; sm++)
            for (size_t p = 0; p < s.P; p++) {
                const size_t src = (sm * frame_px + (size_t)s.pixels[p]) * 2, dst = (sm * s.P + p) * 2;
                jc[dst] = f->jitter[src];
                jc[dst + 1] = f->jitter[src + 1];
            }
        BHG_TRY(s.jitter_d.ensure(s.device, jc.size() * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(s.jitter_d.p, jc.data(), jc.size() * sizeof(double), hipMemcpyHostToDevice, s.stream));
    }
    bhg::RaygenArgs a;
    std::memset(&a, 0, sizeof(a));
    a.jitter = f->jitter.empty() ? nullptr : s.jitter_d.as<double>();
    a.compact = 1;
    a.pixels = s.pixels_d.as<int64_t>();
    a.k0 = s.k0.as<double>();
    a.n_pixels = s.P;
    a.width = f->cam.width;
    a.height = f->cam.height;
    a.samples = f->cam.samples;
    a.fov_x = f->cam.fov_x;
    a.fov_y = f->cam.fov_y;
    static const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    a.rotate = std::memcmp(f->cam.rot, eye, sizeof(eye)) != 0;
    std::memcpy(a.rot, f->cam.rot, sizeof(a.rot));
    if (obs) a.obs = *obs;
    HIP_TRY(bhg::launch_raygen(a, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));   // (jc and the pixel list are host temporaries of this call)
    // the shard's draws stay on the device (16 B per ray): a camera that rotates from frame to frame regenerates its rays
    // with one raygen launch, no host-side gather of the stream and no upload
    s.jitter_ready = !f->jitter.empty();
    s.rays_ready = true;
    return BHG_OK;
}

int upload_shard_scene(bhg_frame *f, Shard &s)
{
    HIP_TRY(hipSetDevice(s.device));
    BHG_TRY(s.sky.ensure(s.device, f->sky.size() * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(s.sky.p, f->sky.data(), f->sky.size() * sizeof(float), hipMemcpyHostToDevice, s.stream));
    if (!f->disk_tex.empty()) {
        BHG_TRY(s.disk_tex.ensure(s.device, f->disk_tex.size() * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(s.disk_tex.p, f->disk_tex.data(), f->disk_tex.size() * sizeof(float), hipMemcpyHostToDevice, s.stream));
    } else {
        s.disk_tex.release();
    }
    HIP_TRY(hipStreamSynchronize(s.stream));
    s.scene_ready = true;
    return BHG_OK;
}

int upload_shard_textures(bhg_frame *f, Shard &s)
{
    HIP_TRY(hipSetDevice(s.device));
    for (int j = 0; j < BHG_MAX_SPHERES; j++) {
        const std::vector<float> &t = f->otex[j];
        if (t.empty()) {
            s.otex[j].release();
            continue;
        }
        BHG_TRY(s.otex[j].ensure(s.device, t.size() * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(s.otex[j].p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, s.stream));
    }
    HIP_TRY(hipStreamSynchronize(s.stream));
    s.otex_ready = true;
    return BHG_OK;
}

void release_shard_instances(Shard &s)
{
    if (s.inst) bhg_mesh_instances_destroy(s.inst);
    s.inst = nullptr;
    s.inst_n = 0;
    s.inst_leaf = 0;
    s.inst_rgb.release();
    s.inst_id.release();
    s.inst_ready = false;
}

void release_shard_mesh(Shard &s, bool keep_tree = false)
{
    if (!keep_tree) {
        release_shard_instances(s);     // (a set does not outlive its mesh)
        if (s.mesh) bhg_mesh_destroy(s.mesh);
        s.mesh = nullptr;
    }
    for (DevBuf *b : {&s.m_rgb, &s.m_uv, &s.m_slot, &s.tri, &s.bary}) b->release();
    for (DevBuf &b : s.m_img) b.release();
    s.mesh_ready = s.mesh_refit = false;
}

// the frame's mesh on this shard's device: the tree is built by bhg_mesh_create, once per device (mesh_bvh.h hands its tree to
// nobody but that call), the material's arrays and images go up beside it
int upload_shard_mesh(bhg_frame *f, Shard &s)
{
    const bhg_frame::Mesh &m = f->mesh;
    const size_t nv = m.vertices.size() / 3, nt = m.triangles.size() / 3;
    const double *normals = m.normals.empty() ? nullptr : m.normals.data();
    // with the device build on, a mesh this device holds takes the new arrays in place when they fit its capacity (section 23)
    bool in_place = false;
    if (f->mesh_build_device && s.mesh && s.mesh_leaf == m.leaf_size && s.mesh_normals == (normals != nullptr)) {
        size_t cap_v = 0, cap_t = 0;
        BHG_TRY(bhg_mesh_build_info(s.mesh, nullptr, nullptr, &cap_v, &cap_t, nullptr));
        in_place = nv <= cap_v && nt <= cap_t;
    }
    release_shard_mesh(s, in_place);
    HIP_TRY(hipSetDevice(s.device));
    if (in_place) {
        HIP_TRY(hipStreamSynchronize(s.stream));    // (no kernel of an earlier render still reads the mesh)
        BHG_TRY(bhg_mesh_rebuild(s.ctx, s.mesh, m.vertices.data(), nv, m.triangles.data(), nt, normals));
        s.inst_ready = false;
    } else if (f->mesh_build_device) {
        // (room to grow: a mesh whose triangle list changes seldom keeps its counts)
        const size_t most = 0x7FFFFFFFull;
        const size_t cap_v = std::min(nv * BHG_FRAME_MESH_HEADROOM, most), cap_t = std::min(nt * BHG_FRAME_MESH_HEADROOM, most);
        BHG_TRY(bhg::mesh_create_built_on_device(s.ctx, m.vertices.data(), nv, m.triangles.data(), nt, normals, m.leaf_size, cap_v, cap_t,
                                                 true, (hipStream_t)bhg_context_stream(s.ctx), &s.mesh));
    } else {
        BHG_TRY(bhg_mesh_create(s.ctx, m.vertices.data(), nv, m.triangles.data(), nt, normals, m.leaf_size, &s.mesh));
    }
    s.mesh_leaf = m.leaf_size;
    s.mesh_normals = normals != nullptr;
    HIP_TRY(hipSetDevice(s.device));
    const auto up = [&](DevBuf &b, const void *src, size_t bytes) -> int {
        if (bytes == 0) return BHG_OK;
        BHG_TRY(b.ensure(s.device, bytes));
        HIP_TRY(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s.stream));
        return BHG_OK;
    };
    BHG_TRY(up(s.m_rgb, m.tri_rgb.data(), m.tri_rgb.size() * sizeof(float)));
    BHG_TRY(up(s.m_uv, m.tri_uv.data(), m.tri_uv.size() * sizeof(float)));
    BHG_TRY(up(s.m_slot, m.tri_tex.data(), m.tri_tex.size() * sizeof(int32_t)));
    for (int j = 0; j < m.n_tex; j++) BHG_TRY(up(s.m_img[j], m.img[j].data(), m.img[j].size() * sizeof(float)));
    HIP_TRY(hipStreamSynchronize(s.stream));
    s.mesh_ready = true;
    s.mesh_refit = false;
    return BHG_OK;
}

// New vertices into the shard's mesh (bhg_frame_refit_mesh): the tree is refitted on the device; past the
// rebuild ratio this device builds it anew from the held triangles.  The material's buffers stay as they are.  An instance set
// over the mesh is set again (a rebuilt mesh: made again) by upload_shard_instances, which the render runs next.
int refit_shard_mesh(bhg_frame *f, Shard &s)
{
    const bhg_frame::Mesh &m = f->mesh;
    const double *normals = m.normals.empty() ? nullptr : m.normals.data();
    const double ratio = m.rebuild_ratio;
    HIP_TRY(hipSetDevice(s.device));
    HIP_TRY(hipStreamSynchronize(s.stream));    // (no kernel of an earlier render still reads the mesh)
    bool rebuild = ratio > 0.0 && ratio <= 1.0;         // (a ratio of 1 or below: always)
    if (!rebuild) {
        BHG_TRY(bhg_mesh_refit(s.ctx, s.mesh, m.vertices.data(), normals));
        double built = 0.0, now = 0.0;
        BHG_TRY(bhg_mesh_refit_info(s.mesh, nullptr, &built, &now));
        rebuild = ratio > 0.0 && built > 0.0 && now > ratio * built;
    }
    if (rebuild && f->mesh_build_device) {
        // in place, on the device: the set over the mesh goes stale and is set again by upload_shard_instances
        BHG_TRY(bhg_mesh_rebuild(s.ctx, s.mesh, m.vertices.data(), m.vertices.size() / 3, m.triangles.data(), m.triangles.size() / 3,
                                 normals));
    } else if (rebuild) {
        release_shard_instances(s);     // (a set does not outlive its mesh)
        bhg_mesh_destroy(s.mesh);
        s.mesh = nullptr;
        s.mesh_ready = false;
        BHG_TRY(bhg_mesh_create(s.ctx, m.vertices.data(), m.vertices.size() / 3, m.triangles.data(), m.triangles.size() / 3, normals,
                                m.leaf_size, &s.mesh));
        s.mesh_ready = true;
    }
    HIP_TRY(hipSetDevice(s.device));
    s.inst_ready = false;
    s.mesh_refit = false;
    return BHG_OK;
}

// the frame's instances on this shard's device, over the shard's mesh: a set of the same size is moved (the records go up,
// nothing else), another size or kind makes a new set
int upload_shard_instances(bhg_frame *f, Shard &s)
{
    const int32_t n = (int32_t)(f->inst.size() / 12);
    HIP_TRY(hipSetDevice(s.device));
    if (s.inst && s.inst_n == n && s.inst_leaf == f->inst_leaf) {
        BHG_TRY(bhg_mesh_instances_set(s.inst, f->inst.data()));
    } else {
        release_shard_instances(s);
        if (f->inst_leaf)
            BHG_TRY(bhg_mesh_instances_create_tree(s.ctx, s.mesh, n, f->inst.data(), f->inst_leaf, &s.inst));
        else
            BHG_TRY(bhg_mesh_instances_create(s.ctx, s.mesh, n, f->inst.data(), &s.inst));
        s.inst_n = n;
        s.inst_leaf = f->inst_leaf;
    }
    HIP_TRY(hipSetDevice(s.device));
    if (f->inst_rgb.empty()) {
        s.inst_rgb.release();
    } else {
        BHG_TRY(s.inst_rgb.ensure(s.device, f->inst_rgb.size() * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(s.inst_rgb.p, f->inst_rgb.data(), f->inst_rgb.size() * sizeof(float), hipMemcpyHostToDevice, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
    }
    s.inst_ready = true;
    return BHG_OK;
}

// the frame's material as the shade call takes it, on this shard's device
void fill_mesh_material(const bhg_frame *f, const Shard &s, bhg_mesh_material *mat)
{
    const bhg_frame::Mesh &m = f->mesh;
    std::memset(mat, 0, sizeof(*mat));
    mat->tri_rgb = m.tri_rgb.empty() ? nullptr : s.m_rgb.as<float>();
    mat->tri_uv = m.tri_uv.empty() ? nullptr : s.m_uv.as<float>();
    mat->tri_tex = m.tri_tex.empty() ? nullptr : s.m_slot.as<int32_t>();
    for (int j = 0; j < m.n_tex; j++) {
        mat->tex[j] = s.m_img[j].as<float>();
        mat->tex_w[j] = m.img_w[j];
        mat->tex_h[j] = m.img_h[j];
    }
    mat->n_tex = m.n_tex;
    mat->emission = m.emission;
}

// the frame's object textures as the shade call takes them: tex = the shard's device copies (s = nullptr: the host copies,
// for the checks before a render)
void fill_object_textures(const bhg_frame *f, const Shard *s, bhg_object_textures *ot)
{
    *ot = f->ot;
    for (int j = 0; j < BHG_MAX_SPHERES; j++) {
        const bool has = !f->otex[j].empty();
        ot->tex[j] = !has ? nullptr : (s ? s->otex[j].as<float>() : f->otex[j].data());
        ot->tex_w[j] = has ? f->otex_w[j] : 0;
        ot->tex_h[j] = has ? f->otex_h[j] : 0;
    }
}

int build_root(bhg_frame *f)
{
    // receive block, frame permutation, image -- on the device of shard 0
    const int root = f->sh[0].device;
    const size_t HW = (size_t)f->cam.width * (size_t)f->cam.height, world = f->sh.size();
    BHG_TRY(f->image.ensure(root, HW * 4 * sizeof(float)));
    if (!f->assembled) {
        HIP_TRY(hipSetDevice(root));
        HIP_TRY(hipEventCreateWithFlags(&f->assembled, hipEventDisableTiming));
    }
    // (a ONE-device frame in RCCL mode sends its slab to itself: the whole gather path on a single GPU, for tests)
    if ((world > 1 && f->gather != BHG_FRAME_GATHER_PEER) || f->gather == BHG_FRAME_GATHER_RCCL) {
        BHG_TRY(f->recv.ensure(root, world * f->pmax * 4 * sizeof(float)));
        BHG_TRY(f->perm.ensure(root, HW * sizeof(int64_t)));
        std::vector<int64_t> perm(HW);
        for (size_t r = 0; r < world; r++)
            for (size_t p = 0; p < f->sh[r].P; p++) perm[(size_t)f->sh[r].pixels[p]] = (int64_t)(r * f->pmax + p);
        HIP_TRY(hipSetDevice(root));
        HIP_TRY(hipMemcpy(f->perm.p, perm.data(), HW * sizeof(int64_t), hipMemcpyHostToDevice));
        for (size_t r = (world > 1 ? 1 : 0); r < world; r++) BHG_TRY(f->sh[r].slab.ensure(f->sh[r].device, f->pmax * 4 * sizeof(float)));
    }
    return BHG_OK;
}

bool is_pinned(const void *p)
{
    hipPointerAttribute_t at;
    if (!p || hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

void fill_scene(const bhg_frame *f, const Shard &s, bhg_scene *sc)
{
    std::memset(sc, 0, sizeof(*sc));
    sc->d_sky = s.sky.as<float>();
    sc->sky_w = f->sky_w;
    sc->sky_h = f->sky_h;
    sc->d_disk_tex = f->disk_tex.empty() ? nullptr : s.disk_tex.as<float>();
    sc->disk_w = f->disk_w;
    sc->disk_h = f->disk_h;
    sc->disk_r_in = f->scene.disk_r_in;
    sc->disk_r_out = f->scene.disk_r_out;
    sc->disk_phase = f->scene.disk_phase;
    sc->disk_mean = f->scene.disk_mean;
    sc->disk_stddev = f->scene.disk_stddev;
    sc->disk_intensity = f->scene.disk_intensity;
    sc->n_spheres = f->scene.n_spheres;
    sc->n_lamps = f->scene.n_lamps;
    std::memcpy(sc->spheres, f->scene.spheres, sizeof(sc->spheres));
    std::memcpy(sc->sphere_rgb, f->scene.sphere_rgb, sizeof(sc->sphere_rgb));
    std::memcpy(sc->lamps, f->scene.lamps, sizeof(sc->lamps));
}

void destroy_frame(bhg_frame *f)
{
    if (!f) return;
    for (auto &s : f->sh) {
        (void)hipSetDevice(s.device);
        if (s.stream) (void)hipStreamSynchronize(s.stream);
    }
    for (auto &s : f->sh)
        if (s.comm && rccl().ok()) (void)rccl().CommDestroy(s.comm);
    for (auto &s : f->sh) {
        (void)hipSetDevice(s.device);
        for (DevBuf *b : {&s.pixels_d, &s.jitter_d, &s.k0, &s.end, &s.dir, &s.flags, &s.steps, &s.acc, &s.obj, &s.slab, &s.sky, &s.disk_tex,
                           &s.start_h, &s.start_rec})
            b->release();
        for (DevBuf &b : s.otex) b.release();
        release_shard_mesh(s);
        if (s.done) (void)hipEventDestroy(s.done);
        for (auto &e : s.evs) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
        if (s.ctx) bhg_destroy(s.ctx);
    }
    f->recv.release();
    f->perm.release();
    f->image.release();
    if (!f->sh.empty()) (void)hipSetDevice(f->sh[0].device);
    for (auto e : f->ev_root)
        if (e) (void)hipEventDestroy(e);
    if (f->assembled) (void)hipEventDestroy(f->assembled);
    for (auto e : f->ev_piece)
        if (e) (void)hipEventDestroy(e);
    if (f->pin) (void)hipHostFree(f->pin);
    delete f;
}

}  // namespace

extern "C" {

int bhg_deal_tiles(int32_t width, int32_t height, int32_t tile, int32_t world, const double *tile_cost, int32_t visit_by_cost,
                   double root_share, int32_t rank, int64_t *pixels, size_t capacity, size_t *n_out)
try {
    if (width <= 0 || height <= 0 || tile <= 0 || world <= 0 || rank < 0 || rank >= world || !n_out || !(root_share > 0.0 && root_share <= 1.0))
        return fail(BHG_E_INVALID, "bad argument");
    if (!bhg::tile_grid_fits(width, height, tile)) return fail(BHG_E_INVALID, "more than 2^31 - 1 tiles");
    std::vector<std::vector<int64_t>> px;
    deal_tiles_into(width, height, tile, world, tile_cost, visit_by_cost != 0, root_share, px);
    const auto &mine = px[(size_t)rank];
    *n_out = mine.size();
    if (pixels) {
        if (capacity < mine.size()) return fail(BHG_E_INVALID, "pixel buffer too small");
        std::memcpy(pixels, mine.data(), mine.size() * sizeof(int64_t));
    }
    return BHG_OK;
} catch (...) {
    return host_exception();
}

int bhg_frame_create(const int32_t *devices, int32_t n_devices, const bhg_camera *cam, const double *jitter, int32_t tile,
                     int32_t gather, bhg_frame **out)
try {
    if (!out) return fail(BHG_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!devices || n_devices < 1 || n_devices > 64) return fail(BHG_E_INVALID, "devices: a list of 1 .. 64 device indices");
    if (!cam) return fail(BHG_E_INVALID, "camera is NULL");
    if (cam->width <= 0 || cam->height <= 0 || cam->samples <= 0) return fail(BHG_E_INVALID, "width, height, samples must be > 0");
    if (tile <= 0) tile = 32;
    if (gather != BHG_FRAME_GATHER_AUTO && gather != BHG_FRAME_GATHER_COPY && gather != BHG_FRAME_GATHER_RCCL &&
        gather != BHG_FRAME_GATHER_PEER && gather != BHG_FRAME_GATHER_COPY_PEERCALL)
        return fail(BHG_E_INVALID, "unknown gather mode");
    const size_t HW = (size_t)cam->width * (size_t)cam->height;
    if (HW * (size_t)cam->samples > 0xFFFFFFFFull) return fail(BHG_E_INVALID, "more than 2^32 rays in the frame");
    if (!bhg::tile_grid_fits(cam->width, cam->height, tile)) return fail(BHG_E_INVALID, "more than 2^31 - 1 tiles");
    const int n_vis = bhg_device_count();
    if (n_vis <= 0) return fail(BHG_E_NO_DEVICE, "no HIP device visible (libbhgeo has no CPU fallback)");
    bool distinct = true;
    for (int i = 0; i < n_devices; i++) {
        if (devices[i] < 0 || devices[i] >= n_vis) return fail(BHG_E_NO_DEVICE, "device index out of range");
        for (int j = 0; j < i; j++) distinct = distinct && devices[i] != devices[j];
    }
    if (gather == BHG_FRAME_GATHER_RCCL && !distinct)
        return fail(BHG_E_INVALID, "RCCL needs distinct devices (a repeated device gathers by device-to-device copies)");
    if (gather == BHG_FRAME_GATHER_RCCL && !rccl().ok()) return fail(BHG_E_HIP, "librccl.so could not be loaded");
    DeviceGuard scope;
    struct Guard {        // (an exception on the way -- the jitter copy, the dealing -- must not leave the half-built frame behind)
        bhg_frame *f = nullptr;
        ~Guard() { if (f) destroy_frame(f); }
    } guard;
    bhg_frame *f = guard.f = new (std::nothrow) bhg_frame();
    if (!f) return fail(BHG_E_NOMEM, "host allocation failed");
    f->cam = *cam;
    f->tile = tile;
    if (gather == BHG_FRAME_GATHER_COPY_PEERCALL) {      // (an explicit mode of the call, not an environment variable: ADVICE r05)
        f->peer_copy_always = true;
        gather = BHG_FRAME_GATHER_COPY;
    }
    std::memset(&f->scene, 0, sizeof(f->scene));
    f->scene.disk_mean = 0.2;   // the Limited engine's defaults (LimitedRelativisticRenderEngine.py:495-498)
    f->scene.disk_stddev = 0.3;
    f->scene.disk_intensity = 1.0;
    if (jitter) f->jitter.assign(jitter, jitter + 2 * HW * (size_t)cam->samples);
    f->sh.resize((size_t)n_devices);
    int rc = BHG_OK;
    for (int i = 0; i < n_devices && rc == BHG_OK; i++) {
        Shard &s = f->sh[i];
        s.device = devices[i];
        rc = bhg_create(s.device, &s.ctx);
        if (rc != BHG_OK) break;
        s.stream = (hipStream_t)bhg_context_stream(s.ctx);
        hipError_t e = hipSetDevice(s.device);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
        if (e != hipSuccess) rc = fail_hip(e, "hipEventCreate");
    }
    // gather mode: RCCL when asked for, or (AUTO) when there is something to gather between distinct devices
    f->gather = BHG_FRAME_GATHER_COPY;
    if (rc == BHG_OK && n_devices > 1 && distinct && gather != BHG_FRAME_GATHER_COPY && gather != BHG_FRAME_GATHER_PEER && rccl().ok())
        f->gather = BHG_FRAME_GATHER_RCCL;
    if (rc == BHG_OK && n_devices == 1 && gather == BHG_FRAME_GATHER_RCCL) f->gather = BHG_FRAME_GATHER_RCCL;   // (a 1-rank group: tests)
    if (rc == BHG_OK && f->gather == BHG_FRAME_GATHER_RCCL) {
        std::vector<nccl_comm_t> comms((size_t)n_devices, nullptr);
        std::vector<int> devs(devices, devices + n_devices);
        const int e = rccl().CommInitAll(comms.data(), n_devices, devs.data());
        if (e != 0) {
            if (gather == BHG_FRAME_GATHER_RCCL) rc = fail_nccl(e, "ncclCommInitAll");
            else f->gather = BHG_FRAME_GATHER_COPY;   // AUTO: fall back to copies
        } else {
            for (int i = 0; i < n_devices; i++) f->sh[i].comm = comms[i];
        }
    }
    if (rc == BHG_OK && gather == BHG_FRAME_GATHER_PEER) f->gather = BHG_FRAME_GATHER_PEER;
    if (rc == BHG_OK && (f->gather == BHG_FRAME_GATHER_COPY || f->gather == BHG_FRAME_GATHER_PEER) && n_devices > 1) {
        // peer access to the first device: for the copies best effort (without it the runtime stages through the host),
        // for the peer stores a must
        for (int i = 1; i < n_devices && rc == BHG_OK; i++) {
            if (devices[i] == devices[0]) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, devices[i], devices[0]) == hipSuccess && can) {
                (void)hipSetDevice(devices[i]);
                hipError_t e = hipDeviceEnablePeerAccess(devices[0], 0);
                if (e != hipSuccess) (void)hipGetLastError();   // (already enabled is fine)
            } else if (f->gather == BHG_FRAME_GATHER_PEER) {
                rc = fail(BHG_E_HIP, "BHG_FRAME_GATHER_PEER: a listed device cannot access the first device's memory");
            }
        }
    }
    if (rc == BHG_OK) {
        deal_tiles(f);
        rc = build_root(f);
    }
    if (rc != BHG_OK) {
        const std::string msg = bhg_last_error();
        guard.f = nullptr;
        destroy_frame(f);
        return fail(rc, msg);
    }
    guard.f = nullptr;
    *out = f;
    return BHG_OK;
} catch (...) {
    return host_exception();
}

void bhg_frame_destroy(bhg_frame *f)
{
    DeviceGuard scope;
    destroy_frame(f);
}

int bhg_frame_set_camera(bhg_frame *f, const bhg_camera *cam)
{
    if (!f || !cam) return fail(BHG_E_INVALID, "frame / camera is NULL");
    if (cam->width != f->cam.width || cam->height != f->cam.height || cam->samples != f->cam.samples)
        return fail(BHG_E_INVALID, "width, height and samples are fixed at bhg_frame_create (the jitter stream and the tile dealing belong to them)");
    // the rays are directions only (the origin is handed to every trace call): they are regenerated when what shapes them changes
    const bool dirs_change = cam->fov_x != f->cam.fov_x || cam->fov_y != f->cam.fov_y || std::memcmp(cam->rot, f->cam.rot, sizeof(cam->rot)) != 0;
    f->cam = *cam;
    if (dirs_change)
        for (auto &s : f->sh) s.drop_rays();
    return BHG_OK;
}

int bhg_frame_set_scene(bhg_frame *f, const bhg_frame_scene *sc)
try {
    if (!f || !sc) return fail(BHG_E_INVALID, "frame / scene is NULL");
    if (sc->n_spheres < 0 || sc->n_spheres > BHG_MAX_SPHERES || sc->n_lamps < 0 || sc->n_lamps > 4)
        return fail(BHG_E_INVALID, "n_spheres must be in [0, BHG_MAX_SPHERES], n_lamps in [0, 4]");
    if (sc->sky && (sc->sky_w <= 0 || sc->sky_h <= 0)) return fail(BHG_E_INVALID, "sky size must be > 0");
    if (!sc->sky && f->sky.empty()) return fail(BHG_E_INVALID, "the first scene must bring a sky image");
    if (sc->disk_r_out > 0.0 && (!(sc->disk_r_out > sc->disk_r_in) || !(sc->disk_r_in >= 0.0) || !(sc->disk_stddev > 0.0)))
        return fail(BHG_E_INVALID, "disk needs 0 <= r_in < r_out and stddev > 0");
    if (sc->disk_tex && (sc->disk_w <= 0 || sc->disk_h <= 0)) return fail(BHG_E_INVALID, "disk texture size must be > 0");
    for (int j = 0; j < sc->n_spheres; j++)
        if (!(sc->spheres[j][3] > 0.0)) return fail(BHG_E_INVALID, "sphere radii must be > 0");
    bool images_changed = false;
    if (sc->sky) {
        f->sky.assign(sc->sky, sc->sky + (size_t)sc->sky_w * (size_t)sc->sky_h * 4);
        f->sky_w = sc->sky_w;
        f->sky_h = sc->sky_h;
        images_changed = true;
    }
    if (sc->disk_tex) {
        f->disk_tex.assign(sc->disk_tex, sc->disk_tex + (size_t)sc->disk_w * (size_t)sc->disk_h * 4);
        f->disk_w = sc->disk_w;
        f->disk_h = sc->disk_h;
        images_changed = true;
    } else if (!(sc->disk_r_out > 0.0) && !f->disk_tex.empty()) {
        f->disk_tex.clear();
        f->disk_w = f->disk_h = 0;
        images_changed = true;
    }
    f->scene = *sc;
    f->scene.sky = f->scene.disk_tex = nullptr;   // (no pointer of the caller's is kept)
    if (images_changed)
        for (auto &s : f->sh) s.scene_ready = false;
    return BHG_OK;
} catch (...) {
    return host_exception();
}

int bhg_frame_set_redshift(bhg_frame *f, const bhg_redshift *rs)
{
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    if (!rs || rs->apply == 0) {
        f->rs.apply = 0;
        return BHG_OK;
    }
    // what can be checked without the trace parameters (the metric and the disk are checked at every render)
    if (rs->apply & ~(BHG_REDSHIFT_DISK | BHG_REDSHIFT_OBJECTS | BHG_REDSHIFT_SKY))
        return fail(BHG_E_INVALID, "redshift apply has bits outside BHG_REDSHIFT_DISK | _OBJECTS | _SKY: " + std::to_string(rs->apply));
    if (!std::isfinite(rs->exponent)) return fail(BHG_E_INVALID, "redshift exponent is not finite");
    if (rs->disk_sense != 1 && rs->disk_sense != -1)
        return fail(BHG_E_INVALID, "redshift disk_sense must be +1 or -1, not " + std::to_string(rs->disk_sense));
    f->rs = *rs;
    return BHG_OK;
}

int bhg_frame_set_observer(bhg_frame *f, const bhg_observer *obs)
{
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    if (obs) {
        // what can be checked without the trace parameters (the metric, the horizon and the axis are checked at every render)
        const double *b = obs->beta;
        if (!(std::isfinite(b[0]) && std::isfinite(b[1]) && std::isfinite(b[2])) || !(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] < 1.0))
            return fail(BHG_E_INVALID, "observer beta must be finite with |beta| < 1");
        f->obs = *obs;
    }
    f->observer = obs != nullptr;
    // the rays of the devices were made for the previous camera model: make them anew at the next render
    for (auto &s : f->sh) s.drop_rays();
    return BHG_OK;
}

int bhg_frame_set_disk_thermal(bhg_frame *f, const bhg_disk_thermal *th)
{
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    if (th) {
        // what can be checked without the trace parameters (the metric, the disk and the camera are checked at every render)
        BHG_TRY(bhg::thermal_check(th));
        f->th = *th;
    }
    f->thermal = th != nullptr;
    return BHG_OK;
}

int bhg_frame_set_object_motion(bhg_frame *f, const bhg_object_motion *mo)
{
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    if (mo) {
        // against the scene's spheres as they are now (the horizon and the timelike bound need the metric: checked at every render)
        BHG_TRY(bhg::motion_check(mo, f->scene.n_spheres));
        f->mo = *mo;
    }
    f->moving = mo != nullptr;
    return BHG_OK;
}

int bhg_frame_set_object_textures(bhg_frame *f, const bhg_object_textures *ot)
try {
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    if (!ot) {
        // off: the frame's shading without textures, and the images freed (host and devices)
        f->textured = false;
        std::memset(&f->ot, 0, sizeof(f->ot));
        for (int j = 0; j < BHG_MAX_SPHERES; j++) {
            std::vector<float>().swap(f->otex[j]);
            f->otex_w[j] = f->otex_h[j] = 0;
        }
        DeviceGuard scope;
        for (auto &s : f->sh) {
            for (DevBuf &b : s.otex) b.release();
            s.otex_ready = false;
        }
        return BHG_OK;
    }
    // the checks of the shade call, against the scene as it stands (and again at every render)
    bhg::ObjectTextureParams tp;
    BHG_TRY(bhg::object_texture_params(ot, f->scene.n_spheres, &tp));
    // the new images are copied aside first: a refused host allocation leaves the frame as it was
    const int n = f->scene.n_spheres;
    std::vector<float> fresh[BHG_MAX_SPHERES];
    bool images_changed = false;
    for (int j = 0; j < n; j++)
        if (ot->tex[j]) {
            fresh[j].assign(ot->tex[j], ot->tex[j] + (size_t)ot->tex_w[j] * (size_t)ot->tex_h[j] * 4);
            images_changed = true;
        }
    for (int j = 0; j < n; j++)
        if (ot->tex[j]) {
            f->otex[j].swap(fresh[j]);
            f->otex_w[j] = ot->tex_w[j];
            f->otex_h[j] = ot->tex_h[j];
        }
    f->ot = *ot;
    for (int j = 0; j < BHG_MAX_SPHERES; j++) f->ot.tex[j] = nullptr;   // (no pointer of the caller's is kept)
    f->textured = true;
    // rotations, modes and strengths travel as kernel arguments: only new images are uploaded
    if (images_changed)
        for (auto &s : f->sh) s.otex_ready = false;
    return BHG_OK;
} catch (...) {
    return host_exception();
}

int bhg_frame_set_mesh(bhg_frame *f, const double *vertices, size_t n_vertices, const int32_t *triangles, size_t n_triangles,
                       const double *vertex_normals, int32_t leaf_size, double max_chord, const bhg_mesh_material *material)
try {
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    if (!vertices) {
        // off: the plain render again, the mesh freed (host and devices)
        f->meshed = false;
        f->mesh = bhg_frame::Mesh();
        f->inst.clear();
        f->inst_rgb.clear();
        DeviceGuard scope;
        for (auto &s : f->sh) release_shard_mesh(s);
        return BHG_OK;
    }
    // bhg_mesh_create's checks and the material's, before anything of the frame's changes
    if (const char *why = bhg::mesh_refusal(vertices, n_vertices, triangles, n_triangles, leaf_size)) return fail(BHG_E_INVALID, why);
    BHG_TRY(bhg::mesh_finite_check(nullptr, vertex_normals, n_vertices * 3));     // (the vertices: mesh_refusal)
    if (!std::isfinite(max_chord) || max_chord < 0.0)
        return fail(BHG_E_INVALID, "max_chord must be finite and >= 0 (0: a quarter of r_s)");
    if (f->mesh_build_device && leaf_size > bhg::MORTON_LEAF_MAX)
        return fail(BHG_E_INVALID, "mesh device build: leaf_size must be in [1, 64] while bhg_frame_set_mesh_build is on");
    if (material) BHG_TRY(bhg::mesh_material_check(material, n_triangles, true));
    // the new mesh is copied aside first: a refused host allocation leaves the frame as it was
    bhg_frame::Mesh m;
    const size_t nt = n_triangles;
    m.vertices.assign(vertices, vertices + n_vertices * 3);
    m.triangles.assign(triangles, triangles + nt * 3);
    if (vertex_normals) m.normals.assign(vertex_normals, vertex_normals + n_vertices * 3);
    m.leaf_size = leaf_size;
    m.max_chord = max_chord;
    if (material) {
        if (material->tri_rgb) m.tri_rgb.assign(material->tri_rgb, material->tri_rgb + nt * 3);
        if (material->tri_uv) {
            m.tri_uv.assign(material->tri_uv, material->tri_uv + nt * 6);
            if (material->tri_tex) m.tri_tex.assign(material->tri_tex, material->tri_tex + nt);
            m.n_tex = material->n_tex;
            for (int j = 0; j < m.n_tex; j++) {
                m.img_w[j] = material->tex_w[j];
                m.img_h[j] = material->tex_h[j];
                m.img[j].assign(material->tex[j], material->tex[j] + (size_t)m.img_w[j] * (size_t)m.img_h[j] * 4);
            }
        }
        m.emission = material->emission;
    }
    f->mesh = std::move(m);
    f->meshed = true;
    f->inst.clear();            // (new arrays: the instances are off)
    f->inst_rgb.clear();
    for (auto &s : f->sh) s.mesh_ready = s.inst_ready = false;
    return BHG_OK;
} catch (...) {
    return host_exception();
}

int bhg_frame_refit_mesh(bhg_frame *f, const double *vertices, const double *vertex_normals, double rebuild_ratio)
try {
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    if (!f->meshed) return fail(BHG_E_INVALID, "mesh refit: the frame holds no mesh (bhg_frame_set_mesh first)");
    if (!vertices) return fail(BHG_E_INVALID, "mesh refit: vertices is NULL");
    bhg_frame::Mesh &m = f->mesh;
    if (vertex_normals && m.normals.empty())
        return fail(BHG_E_INVALID, "mesh refit: vertex_normals given to a mesh that was created without them");
    if (!vertex_normals && !m.normals.empty())
        return fail(BHG_E_INVALID, "mesh refit: vertex_normals is NULL for a mesh that was created with them");
    if (std::isnan(rebuild_ratio)) return fail(BHG_E_INVALID, "mesh refit: rebuild_ratio is NaN");
    const size_t n3 = m.vertices.size();
    BHG_TRY(bhg::mesh_finite_check(vertices, vertex_normals, n3));
    std::copy(vertices, vertices + n3, m.vertices.begin());
    if (vertex_normals) std::copy(vertex_normals, vertex_normals + n3, m.normals.begin());
    m.rebuild_ratio = rebuild_ratio;
    // a device that holds the mesh refits it at the next render; one that does not yet uploads the new vertices anyway
    for (auto &s : f->sh) s.mesh_refit = s.mesh_ready;
    return BHG_OK;
} catch (...) {
    return host_exception();
}

// bhg_frame_set_mesh_instances (leaf_size 0: linear sets) and bhg_frame_set_mesh_instance_tree
static int frame_set_instances(bhg_frame *f, int32_t n, const double *transforms, const float *inst_rgb, int32_t leaf_size)
try {
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    if (!f->meshed) return fail(BHG_E_INVALID, "mesh instances: the frame holds no mesh (bhg_frame_set_mesh first)");
    if (n == 0) {
        // off: the plain mesh render again
        f->inst.clear();
        f->inst_rgb.clear();
        DeviceGuard scope;
        for (auto &s : f->sh) release_shard_instances(s);
        return BHG_OK;
    }
    if (leaf_size)
        BHG_TRY(bhg::mesh_instance_tree_check(n, transforms, leaf_size));
    else
        BHG_TRY(bhg::mesh_instance_transforms_check(n, transforms));
    if (inst_rgb)
        for (int32_t i = 0; i < n * 3; i++)
            if (!std::isfinite(inst_rgb[i])) return fail(BHG_E_INVALID, "mesh instances: every entry of inst_rgb must be finite");
    std::vector<double> T(transforms, transforms + (size_t)n * 12);
    std::vector<float> rgb;
    if (inst_rgb) rgb.assign(inst_rgb, inst_rgb + (size_t)n * 3);
    f->inst = std::move(T);
    f->inst_rgb = std::move(rgb);
    f->inst_leaf = leaf_size;
    for (auto &s : f->sh) s.inst_ready = false;
    return BHG_OK;
} catch (...) {
    return host_exception();
}

int bhg_frame_set_mesh_instances(bhg_frame *f, int32_t n, const double *transforms, const float *inst_rgb)
{
    return frame_set_instances(f, n, transforms, inst_rgb, 0);
}

int bhg_frame_set_mesh_instance_tree(bhg_frame *f, int32_t n, const double *transforms, const float *inst_rgb, int32_t leaf_size)
{
    // (n = 0 turns instances off whatever the leaf_size; otherwise a leaf_size outside [1, 8] is refused with the transforms)
    if (n != 0 && leaf_size == 0) leaf_size = -1;
    return frame_set_instances(f, n, transforms, inst_rgb, leaf_size);
}

int bhg_frame_render(bhg_frame *f, const bhg_params *p, float *rgba_host)
try {
    if (!f || !p) return fail(BHG_E_INVALID, "frame / params is NULL");
    if (f->sky.empty()) return fail(BHG_E_INVALID, "bhg_frame_set_scene() first (the frame has no sky)");
    if ((p->disk_r_out > 0.0) != (f->scene.disk_r_out > 0.0) ||
        (p->disk_r_out > 0.0 && (p->disk_r_in != f->scene.disk_r_in || p->disk_r_out != f->scene.disk_r_out)))
        return fail(BHG_E_INVALID, "the disk of the trace parameters and of the scene differ");
    DeviceGuard scope;
    const size_t world = f->sh.size(), HW = (size_t)f->cam.width * (size_t)f->cam.height;
    const int S = f->cam.samples;
    const bool has_obj = f->scene.n_spheres > 0, has_disk = f->scene.disk_r_out > 0.0;
    const bool meshed = f->meshed;
    const bool instanced = meshed && !f->inst.empty();
    if (meshed) {   // (refused before anything is enqueued)
        const char *with = has_obj ? "scene spheres" : f->rs.apply != 0 ? "redshift" : f->thermal ? "the thermal disk"
                           : f->moving ? "object motion" : f->textured ? "object textures" : nullptr;
        if (with) return fail(BHG_E_INVALID, std::string("a mesh does not go with ") + with);
    }
    const bool dir_only = !has_obj && !has_disk && !meshed;
    const bool loopback = world == 1 && f->gather == BHG_FRAME_GATHER_RCCL;   // (see build_root)
    const bool peer = f->gather == BHG_FRAME_GATHER_PEER;     // every device's shade stores straight into the image
    const bool gathered = (world > 1 && !peer) || loopback;
    Shard &root = f->sh[0];
    bhg_params prm = *p;
    if (prm.order_blocks == 0 && S > 1) prm.order_blocks = (uint32_t)S;   // the rays are S blocks of P (sample-major)
    const char *sc_env = std::getenv("BHGEO_START_CACHE");   // "0": every render works the initial steps out (A/B, short memory)
    const bool start_cache = !(sc_env && sc_env[0] == '0' && sc_env[1] == 0);
    const char *sp_env = std::getenv("BHGEO_START_PREFIX");  // "0": the start steps alone, no start-up records (A/B, 112 B per ray less)
    const bool start_prefix = start_cache && !(sp_env && sp_env[0] == '0' && sp_env[1] == 0);
    const char *dp_env = std::getenv("BHGEO_DEEP_PREFIX");   // "0": the records by BHG_PREFIX_RECORD, not BHG_PREFIX_RECORD_DEEP (A/B)
    // the records are written by BHG_PREFIX_RECORD_DEEP and, after a long run of replaying renders, again by BHG_PREFIX_RECORD_WIDE
    // (bhg::PrefixOwner: promote).  BHGEO_WIDE_PREFIX "1": by the wide rule from the first render; "0": never (A/B)
    const char *wp_env = std::getenv("BHGEO_WIDE_PREFIX");
    const bool no_deep = dp_env && dp_env[0] == '0' && dp_env[1] == 0;
    const bool wide_off = wp_env && wp_env[0] == '0' && wp_env[1] == 0, wide_now = wp_env && wp_env[0] == '1' && wp_env[1] == 0;
    // ... and after a further run on wide records by BHG_PREFIX_RECORD_RIM, the next rung of the same ladder.  BHGEO_RIM_PREFIX "1":
    // by the rim rule from the first render; "0": never, the ladder ends at the wide rule as it did before there was a rim rule (A/B)
    const char *rp_env = std::getenv("BHGEO_RIM_PREFIX");
    const bool rim_off = rp_env && rp_env[0] == '0' && rp_env[1] == 0, rim_now = rp_env && rp_env[0] == '1' && rp_env[1] == 0;
    const int32_t record_mode = no_deep   ? BHG_PREFIX_RECORD
                                : rim_now ? BHG_PREFIX_RECORD_RIM
                                : wide_now ? BHG_PREFIX_RECORD_WIDE
                                           : BHG_PREFIX_RECORD_DEEP;
    const int32_t promote_mode = (no_deep || rim_now || wide_off) ? BHG_PREFIX_NONE
                                 : !rim_off                        ? BHG_PREFIX_RECORD_RIM
                                 : wide_now                        ? BHG_PREFIX_NONE
                                                                   : BHG_PREFIX_RECORD_WIDE;
    const bool redshift = f->rs.apply != 0;
    if (redshift) {   // (refused before anything is enqueued)
        bhg::RedshiftParams rp;
        BHG_TRY(bhg::redshift_params(&prm, &f->rs, has_disk && (f->rs.apply & BHG_REDSHIFT_DISK) ? f->scene.disk_r_in : -1.0,
                                     f->cam.origin, &rp));
    }
    bhg::ObserverParams op;
    if (f->observer) {
        BHG_TRY(bhg::observer_params(&prm, &f->obs, f->cam.origin, &op));
        // the tetrad depends on the camera position and the metric: rays made for others are made anew
        const double key[6] = {op.x0[0], op.x0[1], op.x0[2], op.r_s, op.spin, (double)op.rhs};
        if (std::memcmp(key, f->obs_key, sizeof(key)) != 0) {
            for (auto &s : f->sh) s.drop_rays();
            std::memcpy(f->obs_key, key, sizeof(key));
        }
    }
    const bhg_observer *obs = f->observer ? &f->obs : nullptr;
    const bool textured = f->textured && has_obj;
    if (textured) {   // (the table against the scene as it is now, before anything is enqueued)
        bhg_object_textures ot;
        fill_object_textures(f, nullptr, &ot);
        bhg::ObjectTextureParams tp;
        BHG_TRY(bhg::object_texture_params(&ot, f->scene.n_spheres, &tp));
    }
    const bhg_disk_thermal *th = f->thermal ? &f->th : nullptr;
    if (th) {
        bhg::ThermalParams tp;
        bhg::RedshiftParams rp;
        BHG_TRY(bhg::thermal_params(&prm, th, redshift ? &f->rs : nullptr, nullptr, has_disk ? f->scene.disk_r_in : -1.0,
                                    f->cam.origin, &tp, &rp));
    }
    const bhg_object_motion *mo = f->moving && has_obj ? &f->mo : nullptr;
    if (mo) {
        bhg::MotionParams mp;
        BHG_TRY(bhg::motion_params(&prm, mo, &f->scene.spheres[0][0], f->scene.n_spheres, &mp));
    }

    // -- every device: (rays, scene images once) trace, shade + sample mean into its slab ---------------------------
    for (size_t r = 0; r < world; r++) {
        Shard &s = f->sh[r];
        if (!s.rays_ready) BHG_TRY(upload_shard_geometry(f, s, f->observer ? &op : nullptr));
        if (!s.scene_ready) BHG_TRY(upload_shard_scene(f, s));
        if (textured && !s.otex_ready) BHG_TRY(upload_shard_textures(f, s));
        if (meshed && !s.mesh_ready) BHG_TRY(upload_shard_mesh(f, s));
        if (meshed && s.mesh_refit) BHG_TRY(refit_shard_mesh(f, s));
        if (instanced && !s.inst_ready) BHG_TRY(upload_shard_instances(f, s));
    }
    for (size_t r = 0; r < world; r++) {
        Shard &s = f->sh[r];
        if (s.P == 0) continue;
        HIP_TRY(hipSetDevice(s.device));
        // where this shard's pixels go: one device -- straight into the image, in frame order; several -- shard 0 into
        // its part of the receive block, the others into their own slab
        float *dst = !gathered ? f->image.as<float>() : ((r == 0 && !loopback) ? f->recv.as<float>() : s.slab.as<float>());
        const int64_t *scatter = !gathered ? s.pixels_d.as<int64_t>() : nullptr;
        if (f->profiling) {
            if (s.ev_used == s.evs.size()) {
                hipEvent_t e0, e1;
                HIP_TRY(hipEventCreate(&e0));
                HIP_TRY(hipEventCreate(&e1));
                s.evs.emplace_back(e0, e1);
            }
            HIP_TRY(hipEventRecord(s.evs[s.ev_used].first, s.stream));
        }
        if (meshed) {
            // the mesh trace: whole records, its own kernel, the plain call; the shard's kept initial steps and start-up records
            // are neither used nor touched (they are still valid when the mesh is turned off)
            BHG_TRY(s.end.ensure(s.device, s.n * 6 * sizeof(double)));
            BHG_TRY(s.tri.ensure(s.device, s.n * sizeof(int32_t)));
            BHG_TRY(s.bary.ensure(s.device, s.n * 2 * sizeof(double)));
            const double chord = f->mesh.max_chord > 0.0 ? f->mesh.max_chord : 0.25 * prm.r_s;
            // (over the instances: the same two calls in their instanced forms, and the third record)
            if (instanced) {
                BHG_TRY(s.inst_id.ensure(s.device, s.n * sizeof(int32_t)));
                BHG_TRY(bhg_trace_mesh_instances_device(s.ctx, &prm, s.inst, chord, f->cam.origin, nullptr, s.k0.as<double>(), s.n,
                                                        s.end.as<double>(), s.flags.as<uint8_t>(), s.steps.as<uint32_t>(),
                                                        s.acc.as<uint32_t>(), s.tri.as<int32_t>(), s.inst_id.as<int32_t>(),
                                                        s.bary.as<double>(), s.stream));
            } else {
                BHG_TRY(bhg_trace_mesh_device(s.ctx, &prm, s.mesh, chord, f->cam.origin, nullptr, s.k0.as<double>(), s.n,
                                              s.end.as<double>(), s.flags.as<uint8_t>(), s.steps.as<uint32_t>(), s.acc.as<uint32_t>(),
                                              s.tri.as<int32_t>(), s.bary.as<double>(), s.stream));
            }
            if (f->profiling) HIP_TRY(hipEventRecord(s.evs[s.ev_used++].second, s.stream));
            bhg_scene sc;
            fill_scene(f, s, &sc);
            bhg_mesh_material mat;
            fill_mesh_material(f, s, &mat);
            if (instanced) {
                BHG_TRY(bhg_shade_mesh_instances_device(s.ctx, s.end.as<double>(), s.flags.as<uint8_t>(), s.tri.as<int32_t>(),
                                                        s.inst_id.as<int32_t>(), s.bary.as<double>(), s.P, S, &sc, s.inst, &mat,
                                                        f->inst_rgb.empty() ? nullptr : s.inst_rgb.as<float>(), nullptr, dst, scatter,
                                                        s.stream));
            } else {
                BHG_TRY(bhg_shade_mesh_material_device(s.ctx, s.end.as<double>(), s.flags.as<uint8_t>(), s.tri.as<int32_t>(),
                                                       s.bary.as<double>(), s.P, S, &sc, s.mesh, &mat, nullptr, dst, scatter, s.stream));
            }
            s.dir_traced = false;
            continue;
        }
        // The shard owns its rays, so their initial steps outlive the render: recorded by the first trace of a ray set,
        // replayed while the rays, the origin and what bhg_start_steps_match() lists stay as they were.  Not valid while a
        // call is being issued: a failed enqueue leaves it so.
        int32_t start_mode = BHG_START_NONE;
        if (start_cache) {
            const bool keep = s.start_ready && bhg_start_steps_match(&s.start_prm, &prm) &&
                              std::memcmp(s.start_origin, f->cam.origin, sizeof(s.start_origin)) == 0;
            s.start_ready = false;
            BHG_TRY(s.start_h.ensure(s.device, s.n * sizeof(double)));
            start_mode = keep ? BHG_START_REPLAY : BHG_START_RECORD;
        }
        // ... and so do their start-up records: written by the render that records the steps, handed to every later one with
        // their rho -- the library holds each render's scene against it (an object sphere may have moved in) and says in
        // pf.used what it did.  A scene that stays inside the ball, or one that has left a small ball far behind, has them
        // written again by a render that replays its steps (bhg::PrefixOwner has the rules).
        bhg_prefix pf = {nullptr, 0.0, BHG_PREFIX_NONE, BHG_PREFIX_NONE};
        if (start_prefix) {
            BHG_TRY(s.start_rec.ensure(s.device, s.n * (size_t)BHG_PREFIX_BYTES_PER_RAY));
            pf.d_records = s.start_rec.as<char>();
            if (start_mode == BHG_START_RECORD) {
                s.start_owner = bhg::PrefixOwner();
                pf.mode = record_mode;
            } else {
                const double *sph = has_obj ? &f->scene.spheres[0][0] : nullptr;
                const int32_t n_sph = has_obj ? f->scene.n_spheres : 0;
                // (r_s is the horizon of every call that writes records: a Kerr render holds none, and none is NONE at once)
                pf.mode = s.start_owner.next(record_mode, bhg_prefix_clearance(&prm, sph, n_sph, f->cam.origin), prm.r_s, f->cam.origin,
                                             n_sph, s.start_last.mode, s.start_last.used, s.start_last.rho, promote_mode);
                pf.mode = bhg::prefix_owner_fit_budget(pf.mode, s.start_owner.rho, prm.r_s, f->cam.origin,
                                                       prm.max_steps ? prm.max_steps : (1ull << 20));
                pf.rho = s.start_owner.rho;
            }
        } else {
            s.start_owner = bhg::PrefixOwner();
        }
        if (dir_only) BHG_TRY(s.dir.ensure(s.device, s.n * 3 * sizeof(double)));
        else BHG_TRY(s.end.ensure(s.device, s.n * 6 * sizeof(double)));
        if (has_obj) BHG_TRY(s.obj.ensure(s.device, s.n));
        BHG_TRY(bhg_trace_prefix_device(s.ctx, &prm, has_obj ? &f->scene.spheres[0][0] : nullptr, has_obj ? f->scene.n_spheres : 0,
                                        f->cam.origin, nullptr, s.k0.as<double>(), s.n, dir_only ? nullptr : s.end.as<double>(),
                                        dir_only ? s.dir.as<double>() : nullptr, s.flags.as<uint8_t>(), s.steps.as<uint32_t>(),
                                        s.acc.as<uint32_t>(), has_obj ? s.obj.as<int8_t>() : nullptr, s.start_h.as<double>(),
                                        start_mode, &pf, s.stream));
        s.start_last = pf;
        if (start_cache) {
            s.start_prm = prm;
            std::memcpy(s.start_origin, f->cam.origin, sizeof(s.start_origin));
            s.start_ready = true;
        }
        if (f->profiling) HIP_TRY(hipEventRecord(s.evs[s.ev_used++].second, s.stream));
        // one shade call whatever the scene: a direction-only frame passes its exit directions (its sky g needs only the
        // camera state), the others their whole end records
        bhg_scene sc;
        fill_scene(f, s, &sc);
        bhg_object_textures ot;
        if (textured) fill_object_textures(f, &s, &ot);
        BHG_TRY(bhg_shade_scene_moving_device(s.ctx, dir_only ? nullptr : s.end.as<double>(), dir_only ? s.dir.as<double>() : nullptr,
                                              s.flags.as<uint8_t>(), has_obj ? s.obj.as<int8_t>() : nullptr, s.P, S, &sc, &prm,
                                              redshift ? &f->rs : nullptr, obs, textured ? &ot : nullptr, f->cam.origin,
                                              s.k0.as<double>(), nullptr, dst, scatter, nullptr, nullptr, th, mo, s.stream));
        s.dir_traced = dir_only;
    }
    // -- ONE gather onto the first device -----------------------------------------------------------------------------
    if (f->profiling) {
        if (f->ev_root.empty()) {
            HIP_TRY(hipSetDevice(root.device));
            f->ev_root.resize(2, nullptr);
            for (auto &e : f->ev_root) HIP_TRY(hipEventCreate(&e));
        }
    }
    if (peer && world > 1) {
        // no exchange at all: the image is complete when every device's shade kernel has retired
        for (size_t r = 1; r < world; r++) {
            if (f->sh[r].P == 0) continue;
            HIP_TRY(hipSetDevice(f->sh[r].device));
            HIP_TRY(hipEventRecord(f->sh[r].done, f->sh[r].stream));
        }
        HIP_TRY(hipSetDevice(root.device));
        if (f->profiling) HIP_TRY(hipEventRecord(f->ev_root[0], root.stream));
        for (size_t r = 1; r < world; r++)
            if (f->sh[r].P) HIP_TRY(hipStreamWaitEvent(root.stream, f->sh[r].done, 0));
        if (f->profiling) HIP_TRY(hipEventRecord(f->ev_root[1], root.stream));
    }
    if (gathered) {
        const size_t slab_floats = f->pmax * 4;
        if (f->gather == BHG_FRAME_GATHER_RCCL) {
            // grouped point-to-point: every device sends its slab, the root receives them side by side
            if (f->profiling) {
                HIP_TRY(hipSetDevice(root.device));
                HIP_TRY(hipEventRecord(f->ev_root[0], root.stream));
            }
            NCCL_TRY(rccl().GroupStart());
            int ne = 0;
            const char *what = "";
            for (size_t r = loopback ? 0 : 1; r < world && ne == 0; r++) {
                ne = rccl().Send(f->sh[r].slab.p, slab_floats, NCCL_FLOAT32, 0, f->sh[r].comm, f->sh[r].stream);
                what = "ncclSend";
                if (ne != 0) break;
                ne = rccl().Recv(f->recv.as<float>() + r * slab_floats, slab_floats, NCCL_FLOAT32, (int)r, root.comm, root.stream);
                what = "ncclRecv";
            }
            // (the group is closed on the error path too: a group left open would swallow the next frame's calls)
            const int ge = rccl().GroupEnd();
            if (ne != 0) return fail_nccl(ne, what);
            NCCL_TRY(ge);
        } else {
            for (size_t r = 1; r < world; r++) {
                Shard &s = f->sh[r];
                HIP_TRY(hipSetDevice(s.device));
                // (the root must have read the previous render's slabs out of the receive block)
                if (f->renders > 0) HIP_TRY(hipStreamWaitEvent(s.stream, f->assembled, 0));
                float *dst = f->recv.as<float>() + r * slab_floats;
                if (s.device == root.device && !f->peer_copy_always)
                    HIP_TRY(hipMemcpyAsync(dst, s.slab.p, slab_floats * sizeof(float), hipMemcpyDeviceToDevice, s.stream));
                else
                    HIP_TRY(hipMemcpyPeerAsync(dst, root.device, s.slab.p, s.device, slab_floats * sizeof(float), s.stream));
                HIP_TRY(hipEventRecord(s.done, s.stream));
            }
            HIP_TRY(hipSetDevice(root.device));
            if (f->profiling) HIP_TRY(hipEventRecord(f->ev_root[0], root.stream));
            for (size_t r = 1; r < world; r++) HIP_TRY(hipStreamWaitEvent(root.stream, f->sh[r].done, 0));
        }
        HIP_TRY(hipSetDevice(root.device));
        BHG_TRY(bhg_assemble_frame_f32_device(root.ctx, f->recv.as<float>(), f->perm.as<int64_t>(), HW, f->image.as<float>(), root.stream));
        HIP_TRY(hipEventRecord(f->assembled, root.stream));
        if (f->profiling) HIP_TRY(hipEventRecord(f->ev_root[1], root.stream));
    }
    // -- one array back -----------------------------------------------------------------------------------------------
    HIP_TRY(hipSetDevice(root.device));
    if (rgba_host) {
        const size_t bytes = HW * 4 * sizeof(float);
        if (is_pinned(rgba_host)) {
            HIP_TRY(hipMemcpyAsync(rgba_host, f->image.p, bytes, hipMemcpyDeviceToHost, root.stream));
            HIP_TRY(hipStreamSynchronize(root.stream));
        } else {
            if (f->pin_bytes < bytes) {
                if (f->pin) HIP_TRY(hipHostFree(f->pin));
                f->pin = nullptr;
                f->pin_bytes = 0;
                HIP_TRY(hipHostMalloc(&f->pin, bytes, hipHostMallocDefault));
                f->pin_bytes = bytes;
            }
            // in two halves: while the second half crosses PCIe the first goes from the staging block into the caller's array
            // (the context's copy threads, 512-kB jobs so that all of them have work on half a frame).  Measured on one box
            // (scripts/dev/dev_library_frame.py, 1024 x 1024 frame): 1.80 ms in one piece, 1.72 in two, 1.70-1.75 in four;
            // four pieces with the pool's usual 2-MB jobs: 2.15 (two jobs per piece leave six threads idle)
            constexpr int PIECES = 2;
            if (f->ev_piece.empty()) {
                // (all or nothing: a creation that fails half way must not leave null handles behind for the next render)
                hipEvent_t made[PIECES] = {};
                for (int q = 0; q < PIECES; q++) {
                    const hipError_t e = hipEventCreateWithFlags(&made[q], hipEventDisableTiming);
                    if (e != hipSuccess) {
                        for (int r = 0; r < q; r++) (void)hipEventDestroy(made[r]);
                        return fail_hip(e, "hipEventCreateWithFlags (image pieces)");
                    }
                }
                f->ev_piece.assign(made, made + PIECES);
            }
            const size_t piece = ((bytes / PIECES) + 4095) & ~size_t(4095);
            int n_pieces = 0;
            for (size_t off = 0; off < bytes; off += piece, n_pieces++) {
                const size_t len = std::min(piece, bytes - off);
                HIP_TRY(hipMemcpyAsync((char *)f->pin + off, (const char *)f->image.p + off, len, hipMemcpyDeviceToHost, root.stream));
                HIP_TRY(hipEventRecord(f->ev_piece[n_pieces], root.stream));
            }
            int k = 0;
            for (size_t off = 0; off < bytes; off += piece, k++) {
                HIP_TRY(hipEventSynchronize(f->ev_piece[k]));
                bhg::host_copy(root.ctx, (char *)rgba_host + off, (const char *)f->pin + off, std::min(piece, bytes - off), size_t(512) << 10);
            }
        }
        // (the other devices' streams have been waited for through the gather; a frame of ONE device has one stream)
    }
    f->rendered = true;
    f->renders++;
    return BHG_OK;
} catch (...) {
    return host_exception();
}

int bhg_frame_synchronize(bhg_frame *f)
{
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    DeviceGuard scope;
    for (auto &s : f->sh) {
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(hipStreamSynchronize(s.stream));
    }
    return BHG_OK;
}

const float *bhg_frame_device_image(bhg_frame *f) { return f ? f->image.as<float>() : nullptr; }

int bhg_frame_stats(bhg_frame *f, uint64_t out[4])
try {
    if (!f || !out) return fail(BHG_E_INVALID, "bad argument");
    if (!f->rendered) return fail(BHG_E_INVALID, "no render yet");
    DeviceGuard scope;
    const int W = f->cam.width, T = f->tile, tx = (W + T - 1) / T, ty = (f->cam.height + T - 1) / T;
    f->tile_cost.assign((size_t)tx * ty, 0.0);
    uint64_t rays = 0, att = 0, acc = 0, hor = 0;
    std::vector<uint32_t> hs, ha;
    std::vector<uint8_t> hf;
    for (auto &s : f->sh) {
        if (s.n == 0) continue;
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(hipStreamSynchronize(s.stream));
        hs.resize(s.n);
        ha.resize(s.n);
        hf.resize(s.n);
        HIP_TRY(hipMemcpy(hs.data(), s.steps.p, s.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ha.data(), s.acc.p, s.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hf.data(), s.flags.p, s.n, hipMemcpyDeviceToHost));
        rays += s.n;
        for (size_t i = 0; i < s.n; i++) {
            att += hs[i];
            acc += ha[i];
            hor += (hf[i] & BHG_FLAG_HIT_HORIZON) ? 1 : 0;
            const int64_t pix = s.pixels[i % s.P];
            f->tile_cost[(size_t)((pix / W) / T) * tx + (size_t)((pix % W) / T)] += (double)hs[i];
        }
    }
    out[0] = rays;
    out[1] = att;
    out[2] = acc;
    out[3] = hor;
    return BHG_OK;
} catch (...) {
    return host_exception();
}

int bhg_frame_rebalance(bhg_frame *f, double root_share)
try {
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    if (root_share == 0.0) root_share = 1.0;
    if (!(root_share > 0.0 && root_share <= 1.0)) return fail(BHG_E_INVALID, "root_share must be in (0, 1] (0 = 1)");
    uint64_t st[4];
    BHG_TRY(bhg_frame_stats(f, st));   // (fills tile_cost from the last render's attempted steps)
    DeviceGuard scope;
    f->dealt_by_cost = true;
    f->root_share = root_share;
    deal_tiles(f);
    return build_root(f);
} catch (...) {
    return host_exception();
}

int bhg_frame_set_mesh_build(bhg_frame *f, int on_device)
{
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    if (on_device && f->meshed && f->mesh.leaf_size > bhg::MORTON_LEAF_MAX)
        return fail(BHG_E_INVALID, "mesh device build: the frame's mesh has a leaf_size over 64 (bhg_frame_set_mesh with one in [1, 64] first)");
    f->mesh_build_device = on_device != 0;
    return BHG_OK;
}

int bhg_frame_mesh_build_info(const bhg_frame *f, int32_t shard, int32_t *built_on_device, uint64_t *builds, size_t *cap_vertices,
                              size_t *cap_triangles, uint64_t *allocations)
{
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    if (shard < 0 || (size_t)shard >= f->sh.size()) return fail(BHG_E_INVALID, "shard must be in [0, the frame's devices)");
    if (!f->sh[(size_t)shard].mesh) return fail(BHG_E_INVALID, "this device holds no mesh (none set, or no render since)");
    return bhg_mesh_build_info(f->sh[(size_t)shard].mesh, built_on_device, builds, cap_vertices, cap_triangles, allocations);
}

int bhg_frame_mesh_refit_info(const bhg_frame *f, int32_t shard, uint64_t *generation, double *area_build, double *area_now)
{
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    if (shard < 0 || (size_t)shard >= f->sh.size()) return fail(BHG_E_INVALID, "shard must be in [0, the frame's devices)");
    if (!f->sh[(size_t)shard].mesh) return fail(BHG_E_INVALID, "this device holds no mesh (none set, or no render since)");
    return bhg_mesh_refit_info(f->sh[(size_t)shard].mesh, generation, area_build, area_now);
}

int bhg_frame_prefix_info(const bhg_frame *f, int32_t shard, bhg_prefix *last)
{
    if (!f || !last) return fail(BHG_E_INVALID, "bad argument");
    if (shard < 0 || (size_t)shard >= f->sh.size()) return fail(BHG_E_INVALID, "shard must be in [0, the frame's devices)");
    *last = f->sh[(size_t)shard].start_last;
    return BHG_OK;
}

int bhg_frame_info(const bhg_frame *f, int64_t out[8])
{
    if (!f || !out) return fail(BHG_E_INVALID, "bad argument");
    size_t pmin = (size_t)-1;
    for (auto &s : f->sh) pmin = std::min(pmin, s.P);
    out[0] = (int64_t)f->sh.size();
    out[1] = f->gather;
    out[2] = (int64_t)f->pmax;
    out[3] = (int64_t)pmin;
    out[4] = f->tile;
    out[5] = f->dealt_by_cost ? 1 : 0;
    out[6] = (int64_t)f->renders;
    out[7] = (!f->sh.empty() && f->sh[0].dir_traced) ? 1 : 0;
    return BHG_OK;
}

int bhg_frame_set_profiling(bhg_frame *f, int enable)
{
    if (!f) return fail(BHG_E_INVALID, "frame is NULL");
    f->profiling = enable != 0;   // (a flag: may be switched per render, e.g. on for every 4th frame of a timed loop)
    return BHG_OK;
}

int bhg_frame_last_ms(bhg_frame *f, float *trace_ms, float *root_ms)
try {
    if (!f || !trace_ms) return fail(BHG_E_INVALID, "bad argument");
    DeviceGuard scope;
    bool any = false;
    for (size_t r = 0; r < f->sh.size(); r++) {
        Shard &s = f->sh[r];
        trace_ms[r] = 0.0f;
        if (s.ev_used == 0) continue;
        any = true;
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(hipEventSynchronize(s.evs[s.ev_used - 1].second));
        double sum = 0.0;
        for (size_t i = 0; i < s.ev_used; i++) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, s.evs[i].first, s.evs[i].second));
            sum += ms;
        }
        trace_ms[r] = (float)(sum / (double)s.ev_used);
        s.ev_used = 0;
    }
    if (!any) return fail(BHG_E_INVALID, "no profiled render since the last call (bhg_frame_set_profiling)");
    if (root_ms) {
        *root_ms = 0.0f;
        if ((f->sh.size() > 1 || f->gather == BHG_FRAME_GATHER_RCCL) && f->ev_root.size() == 2) {
            HIP_TRY(hipSetDevice(f->sh[0].device));
            HIP_TRY(hipEventSynchronize(f->ev_root[1]));
            HIP_TRY(hipEventElapsedTime(root_ms, f->ev_root[0], f->ev_root[1]));
        }
    }
    return BHG_OK;
} catch (...) {
    return host_exception();
}

}  // extern "C"
