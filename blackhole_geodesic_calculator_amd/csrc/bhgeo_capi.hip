// bhgeo_capi.hip -- the C ABI of libbhgeo.so (declared in include/bhgeo.h).
//
// Each entry point replaces a piece of the reference's per-ray Python hand-off
// (raytracer/RelativisticRenderEngine.py:134, :293-313; batched contract of
// raytracer/RelativisticRenderEngineCamEdition.py:225-228).  There is no CPU fallback: every
// compute entry point needs a HIP device and fails with BHG_E_NO_DEVICE / BHG_E_HIP otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cfloat>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "bhgeo_internal.h"
#include "mesh_object.h"
#include "prefix_clearance.h"
#include "trace_call.h"

static_assert(BHG_FLAG_HIT_HORIZON == bhg::BHG_FLAG_HIT_HORIZON_, "flag mismatch");
static_assert(BHG_FLAG_START_INSIDE == bhg::BHG_FLAG_START_INSIDE_, "flag mismatch");
static_assert(BHG_FLAG_REACHED_END == bhg::BHG_FLAG_REACHED_END_, "flag mismatch");
static_assert(BHG_FLAG_EXITED_SPHERE == bhg::BHG_FLAG_EXITED_SPHERE_, "flag mismatch");
static_assert(BHG_FLAG_MAX_STEPS == bhg::BHG_FLAG_MAX_STEPS_, "flag mismatch");
static_assert(BHG_FLAG_STEP_TOO_SMALL == bhg::BHG_FLAG_STEP_TOO_SMALL_, "flag mismatch");
static_assert(BHG_FLAG_NAN == bhg::BHG_FLAG_NAN_, "flag mismatch");
static_assert(BHG_FLAG_HIT_OBJECT == bhg::BHG_FLAG_HIT_OBJECT_ && BHG_MAX_SPHERES == bhg::BHG_MAX_SPHERES_, "object constants mismatch");
static_assert(BHG_PREFIX_K_MAX == bhg::BHG_PREFIX_K_MAX_ && BHG_PREFIX_DEEP_ACCEPTED == bhg::BHG_PREFIX_DEEP_ACCEPTED_ &&
                  BHG_PREFIX_DEEP_ATTEMPTS == bhg::BHG_PREFIX_DEEP_ATTEMPTS_ && BHG_PREFIX_DEEP_ACCEPTED <= BHG_PREFIX_DEEP_ATTEMPTS,
              "start-up record limits mismatch");
static_assert(BHG_PREFIX_WIDE_ACCEPTED == bhg::BHG_PREFIX_WIDE_ACCEPTED_ && BHG_PREFIX_DEEP_ACCEPTED <= BHG_PREFIX_WIDE_ACCEPTED &&
                  BHG_PREFIX_WIDE_ACCEPTED <= BHG_PREFIX_DEEP_ATTEMPTS,
              "wide start-up record limits mismatch");
static_assert(BHG_PREFIX_NONE == bhg::PREFIX_MODE_NONE && BHG_PREFIX_RECORD == bhg::PREFIX_MODE_RECORD &&
                  BHG_PREFIX_REPLAY == bhg::PREFIX_MODE_REPLAY && BHG_PREFIX_RECORD_DEEP == bhg::PREFIX_MODE_RECORD_DEEP &&
                  BHG_PREFIX_RECORD_WIDE == bhg::PREFIX_MODE_RECORD_WIDE && BHG_PREFIX_RECORD_RIM == bhg::PREFIX_MODE_RECORD_RIM,
              "start-up record modes mismatch");
static_assert(BHG_PREFIX_RIM_ACCEPTED == bhg::BHG_PREFIX_RIM_ACCEPTED_ && BHG_PREFIX_RIM_ATTEMPTS == bhg::BHG_PREFIX_RIM_ATTEMPTS_ &&
                  BHG_PREFIX_RIM_ACCEPTED == bhg::PREFIX_RIM_ACCEPTED && BHG_PREFIX_RIM_ATTEMPTS == bhg::PREFIX_RIM_ATTEMPTS &&
                  BHG_PREFIX_WIDE_ACCEPTED <= BHG_PREFIX_RIM_ACCEPTED && BHG_PREFIX_RIM_ACCEPTED <= BHG_PREFIX_RIM_ATTEMPTS &&
                  BHG_PREFIX_DEEP_ATTEMPTS <= BHG_PREFIX_RIM_ATTEMPTS,
              "rim start-up record limits mismatch");
static_assert(BHG_METHOD_DP54 == bhg::BHG_METHOD_DP54_ && BHG_METHOD_RK4 == bhg::BHG_METHOD_RK4_, "method mismatch");
static_assert(BHG_RHS_CHRISTOFFEL == bhg::BHG_RHS_CHRISTOFFEL_ && BHG_RHS_REDUCED == bhg::BHG_RHS_REDUCED_ &&
                  BHG_RHS_KERR_BL == bhg::BHG_RHS_KERR_BL_,
              "rhs mismatch");
static_assert(sizeof(bhg_params) == 104, "bhg_params layout is part of the ABI");
static_assert(sizeof(bhg_camera) == 128, "bhg_camera layout is part of the ABI");
static_assert(sizeof(bhg_scene) == 664 && sizeof(bhg_frame_scene) == 664, "scene layouts are part of the ABI");
static_assert(BHG_FLAG_HIT_DISK == bhg::BHG_FLAG_HIT_DISK_, "flag mismatch");
static_assert(BHG_REDSHIFT_DISK == bhg::BHG_REDSHIFT_DISK_ && BHG_REDSHIFT_OBJECTS == bhg::BHG_REDSHIFT_OBJECTS_ &&
                  BHG_REDSHIFT_SKY == bhg::BHG_REDSHIFT_SKY_,
              "redshift class mismatch");
static_assert(sizeof(bhg_redshift) == 16, "bhg_redshift layout is part of the ABI");
static_assert(sizeof(bhg_observer) == 24, "bhg_observer layout is part of the ABI");
static_assert(sizeof(bhg_object_textures) == 800, "bhg_object_textures layout is part of the ABI");
static_assert(sizeof(bhg_polarisation) == 544 && BHG_POL_TABLE_MAX == bhg::BHG_POL_TABLE_MAX_, "bhg_polarisation layout is part of the ABI");
static_assert(sizeof(bhg_disk_thermal) == 544 && BHG_THERMAL_NU_MAX == bhg::BHG_THERMAL_NU_MAX_, "bhg_disk_thermal layout is part of the ABI");
static_assert(sizeof(bhg_object_motion) == 384, "bhg_object_motion layout is part of the ABI");
static_assert(sizeof(bhg_disk_layers) == 16 && BHG_MAX_CROSSINGS == bhg::BHG_MAX_CROSSINGS_, "bhg_disk_layers layout is part of the ABI");
static_assert(BHG_OBJECT_LIT == bhg::BHG_OBJECT_LIT_ && BHG_OBJECT_EMISSIVE == bhg::BHG_OBJECT_EMISSIVE_, "object mode mismatch");

namespace {
thread_local std::string g_err = "";
}  // namespace

namespace bhg {
// for every translation unit of the library (bhgeo_internal.h: fail, fail_hip): the thread-local message of bhg_last_error()
int set_error(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}
}  // namespace bhg

namespace {

// Worker threads for the host side of the host-buffer entry points: a 100-MB-class memcpy between a caller's
// pageable array and the pinned staging ring runs at one core's ~10 GB/s single-threaded, several times below what
// the PCIe link moves; split over a few threads it keeps up.  Created on first use, joined with the context.
class HostCopyPool {
public:
    ~HostCopyPool()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    // dst <- src, blocking; the calling thread takes pieces too
    void copy(void *dst, const void *src, size_t bytes, size_t piece = size_t(2) << 20)
    {
        if (bytes <= 2 * piece) {
            std::memcpy(dst, src, bytes);
            return;
        }
        start();
        size_t n_jobs = 0;
        {
            std::lock_guard<std::mutex> g(m_);
            for (size_t off = 0; off < bytes; off += piece, n_jobs++)
                q_.push_back({(char *)dst + off, (const char *)src + off, std::min(piece, bytes - off)});
            pending_ += n_jobs;
        }
        cv_.notify_all();
        for (;;) {  // help until the queue is empty, then wait for the pieces still being copied
            Job j;
            {
                std::unique_lock<std::mutex> g(m_);
                if (q_.empty()) {
                    done_.wait(g, [&] { return pending_ == 0; });
                    return;
                }
                j = q_.front();
                q_.pop_front();
            }
            std::memcpy(j.dst, j.src, j.bytes);
            finish_one();
        }
    }

private:
    struct Job {
        char *dst;
        const char *src;
        size_t bytes;
    };
    void start()
    {
        if (started_) return;
        started_ = true;
        unsigned hw = std::thread::hardware_concurrency();
        unsigned n = hw > 1 ? std::min(hw - 1, 7u) : 0u;  // + the calling thread
        // (a process at its thread limit: fewer workers, or none -- the calling thread copies what nobody else takes)
        for (unsigned i = 0; i < n; i++) {
            try {
                th_.emplace_back([this] { run(); });
            } catch (const std::exception &) {
                break;
            }
        }
    }
    void finish_one()
    {
        std::lock_guard<std::mutex> g(m_);
        if (--pending_ == 0) done_.notify_all();
    }
    void run()
    {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return stop_ || !q_.empty(); });
                if (stop_ && q_.empty()) return;
                j = q_.front();
                q_.pop_front();
            }
            std::memcpy(j.dst, j.src, j.bytes);
            finish_one();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::deque<Job> q_;
    size_t pending_ = 0;
    bool stop_ = false, started_ = false;
};

}  // namespace

struct bhg_context {
    int device = 0;
    hipStream_t stream = nullptr;
    // work counters (device): two sets of 8 slice counters, one 256-byte line each.  Consecutive launches alternate
    // between the sets; a launch zeroes the set the next one will use (trace kernels, block 0), so no memset launch
    // per call.  counters_clean = both sets are known to be in that state (false after a failed enqueue)
    unsigned long long *counter = nullptr;
    int counter_set = 0;
    bool counters_clean = false;
    hipStream_t last_stream = nullptr;   // the stream of the last trace launch (launches of a context must stay ordered)
    bool launched = false;
    hipEvent_t ev_order = nullptr;
    bool last_stream_foreign = false;    // last_stream is a caller's handle: ev_order was recorded behind that call
    int num_cus = 0;
    char name[256] = {0};
    // device buffers of the host-buffer entry points, grown on demand
    void *d_in = nullptr;
    size_t d_in_bytes = 0;
    void *d_out = nullptr;
    size_t d_out_bytes = 0;
    // their pipeline: copy streams either side of the compute stream, a two-slot pinned staging ring for callers'
    // pageable arrays, events per slot, worker threads for the host-side copies
    hipStream_t s_in = nullptr, s_out = nullptr;
    void *pin_in = nullptr, *pin_out = nullptr;
    size_t pin_in_bytes = 0, pin_out_bytes = 0;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_k[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    HostCopyPool pool;
    // per-ray workspace of a trace call: the flags and step counts its caller does not want
    void *d_ws = nullptr;
    size_t d_ws_bytes = 0;
    void *d_endws = nullptr;   // end records as workspace of direction-only calls
    size_t d_endws_bytes = 0;
    int32_t last_launch[4] = {0, 0, 0, 0};
    int occupancy[96] = {0};  // resident waves per CU of each trace-kernel variant (0 = not asked yet)
    // optional per-pass timing (bhg_set_profiling)
    bool profiling = false;
    bool ev_valid = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // 0, 1 back to back | trace | 2 | (Kerr) finalize | 3
    bool ev_post = false;                                     // the last profiled call had a finalize pass
};

namespace bhg {
// for bhgeo_frame.hip: a context's worker threads copy a page-locked staging block into the caller's pageable array (a
// 16.8-MB frame through ONE thread's memcpy is 1.0-1.7 ms -- as long as the frame's trace)
void host_copy(bhg_context *c, void *dst, const void *src, size_t bytes, size_t piece) { c->pool.copy(dst, src, bytes, piece); }
// for bhgeo_mesh.hip, which sees a context from outside
int context_device(const bhg_context *c) { return c->device; }
hipStream_t context_stream(const bhg_context *c) { return c->stream; }
}  // namespace bhg

namespace {

int ensure(void **p, size_t *have, size_t need)
{
    if (*have >= need) return BHG_OK;
    if (*p) {
        HIP_TRY(hipFree(*p));
        *p = nullptr;
        *have = 0;
    }
    size_t want = need + need / 4 + 4096;
    HIP_TRY(hipMalloc(p, want));
    *have = want;
    return BHG_OK;
}

int ensure_pinned(void **p, size_t *have, size_t need)
{
    if (*have >= need) return BHG_OK;
    if (*p) {
        HIP_TRY(hipHostFree(*p));
        *p = nullptr;
        *have = 0;
    }
    HIP_TRY(hipHostMalloc(p, need, hipHostMallocDefault));
    *have = need;
    return BHG_OK;
}

// Is this host address page-locked memory HIP knows (hipHostMalloc / hipHostRegister, e.g. bhg_host_alloc)?  Then the
// copy engines reach it directly; a pageable array goes through the staging ring.
bool is_pinned(const void *p)
{
    if (!p) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

// ... and a whole range [p, p + bytes): the allocation that holds p must hold its last byte too (hipMemGetAddressRange on
// the device alias of the block); where the runtime cannot tell the extent of a host allocation, both ends must at
// least be page-locked and map to one contiguous device range
bool is_pinned_range(const void *p, size_t bytes, void **dev_out)
{
    if (!p || bytes == 0 || !is_pinned(p)) return false;
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, const_cast<void *>(p), 0) != hipSuccess || !dp) {
        (void)hipGetLastError();
        return false;
    }
    hipDeviceptr_t base = nullptr;
    size_t extent = 0;
    if (hipMemGetAddressRange(&base, &extent, (hipDeviceptr_t)dp) == hipSuccess && base && extent) {
        if ((const char *)dp + bytes > (const char *)base + extent) return false;
    } else {
        (void)hipGetLastError();
        const char *last = (const char *)p + bytes - 1;
        void *dl = nullptr;
        if (!is_pinned(last)) return false;
        if (hipHostGetDevicePointer(&dl, const_cast<char *>(last), 0) != hipSuccess || dl != (char *)dp + bytes - 1) {
            (void)hipGetLastError();
            return false;
        }
    }
    *dev_out = dp;
    return true;
}

// validate_tol (scipy _ivp/common.py:44-51): an rtol below 100 eps is raised to 100 eps -- scipy warns and carries on, and so
// does every solve the reference runs through solve_ivp (README.md:196)
inline double scipy_rtol(double rtol) { return rtol < 100.0 * DBL_EPSILON ? 100.0 * DBL_EPSILON : rtol; }

// What every kernel call takes from bhg_params (validated) and the object spheres: the integration settings, the metric, the
// event radii.  Returns the kernels' right-hand-side id: the time-like Christoffel form is one of its own (the Kerr kernels take
// the norm at the start).  The rays, the outputs, min_step_cap, the work order and the counters are the caller's.
int fill_trace_args(bhg::TraceArgs &a, const bhg_params *p, const double *spheres, int32_t n_spheres)
{
    a.r_s = p->r_s;
    a.lambda_end = p->lambda_end;
    a.max_step = p->max_step;
    a.rtol = scipy_rtol(p->rtol);
    a.atol = p->atol;
    a.h_fixed = p->h_fixed;
    a.r_exit = p->r_exit;
    a.disk_r_in = p->disk_r_in;
    a.disk_r_out = p->disk_r_out;
    a.spin = p->spin;
    a.mu2 = p->time_like ? 1.0 : 0.0;
    a.r_hor = p->r_s;
    if (p->rhs_form == BHG_RHS_KERR_BL) {
        const double M = 0.5 * p->r_s;
        a.r_hor = (M + std::sqrt(M * M - p->spin * p->spin)) * (1.0 + BHG_KERR_HORIZON_MARGIN);
    }
    a.max_steps = p->max_steps ? p->max_steps : (1u << 20);
    a.n_spheres = n_spheres;
    for (int j = 0; j < n_spheres; j++)
        for (int q = 0; q < 4; q++) a.spheres[j][q] = spheres[4 * j + q];
    return (p->time_like && p->rhs_form == BHG_RHS_CHRISTOFFEL) ? bhg::BHG_RHS_CHRISTOFFEL_TL_ : p->rhs_form;
}

int validate(const bhg_params *p)
{
    if (!p) return fail(BHG_E_INVALID, "params is NULL");
    if (!(p->r_s >= 0.0) || !std::isfinite(p->r_s)) return fail(BHG_E_INVALID, "r_s must be finite and >= 0");
    if (!(p->lambda_end >= 0.0) || !std::isfinite(p->lambda_end))
        return fail(BHG_E_INVALID, "lambda_end must be finite and >= 0");
    if (!(p->r_exit >= 0.0) || !std::isfinite(p->r_exit)) return fail(BHG_E_INVALID, "r_exit must be finite and >= 0");
    if (p->method == BHG_METHOD_DP54) {
        if (!(p->max_step > 0.0)) return fail(BHG_E_INVALID, "max_step must be > 0 (use +inf for unset)");
        if (!(p->rtol > 0.0) || !(p->atol > 0.0) || !std::isfinite(p->rtol) || !std::isfinite(p->atol))
            return fail(BHG_E_INVALID, "rtol and atol must be finite and > 0");
    } else if (p->method == BHG_METHOD_RK4) {
        if (!(p->h_fixed > 0.0) || !std::isfinite(p->h_fixed)) return fail(BHG_E_INVALID, "h_fixed must be finite and > 0");
    } else {
        return fail(BHG_E_INVALID, "unknown method");
    }
    if (p->rhs_form != BHG_RHS_CHRISTOFFEL && p->rhs_form != BHG_RHS_REDUCED && p->rhs_form != BHG_RHS_KERR_BL)
        return fail(BHG_E_INVALID, "unknown rhs_form");
    if (p->rhs_form == BHG_RHS_KERR_BL) {
        if (!std::isfinite(p->spin) || !(std::fabs(p->spin) < 0.5 * p->r_s))
            return fail(BHG_E_INVALID, "Kerr needs |spin| < M = r_s/2");
    }
    if (p->time_like != 0 && p->time_like != 1) return fail(BHG_E_INVALID, "time_like must be 0 or 1");
    if (p->time_like && p->rhs_form == BHG_RHS_REDUCED)
        return fail(BHG_E_INVALID, "BHG_RHS_REDUCED is the closed form for null rays: time_like needs BHG_RHS_CHRISTOFFEL or BHG_RHS_KERR_BL");
    if (!(p->disk_r_in >= 0.0) || !(p->disk_r_out >= 0.0) || !std::isfinite(p->disk_r_in) || !std::isfinite(p->disk_r_out))
        return fail(BHG_E_INVALID, "disk radii must be finite and >= 0");
    if (p->disk_r_out > 0.0 && p->disk_r_in > p->disk_r_out) return fail(BHG_E_INVALID, "disk_r_in > disk_r_out");
    return BHG_OK;
}

}  // namespace

namespace bhg {
int params_check(const bhg_params *p) { return validate(p); }   // (for bhgeo_mesh.hip's trace checks)

// The thermal-disk settings on their own (include/bhgeo.h, "the thermal disk"): what can be checked without the trace
// parameters.  Also used by bhgeo_frame.hip.
int thermal_check(const bhg_disk_thermal *th)
{
    if (th->disk_sense != 1 && th->disk_sense != -1)
        return fail(BHG_E_INVALID, "disk thermal disk_sense must be +1 or -1, not " + std::to_string(th->disk_sense));
    if (th->n_nu < 1 || th->n_nu > BHG_THERMAL_NU_MAX)
        return fail(BHG_E_INVALID, "disk thermal n_nu must be in [1, 16], not " + std::to_string(th->n_nu));
    char msg[160];
    for (int j = 0; j < th->n_nu; j++)
        if (!(std::isfinite(th->nu[j]) && th->nu[j] > 0.0)) {
            std::snprintf(msg, sizeof msg, "disk thermal nu[%d] = %.17g must be finite and > 0", j, th->nu[j]);
            return fail(BHG_E_INVALID, msg);
        }
    for (int c = 0; c < 3; c++)
        for (int j = 0; j < th->n_nu; j++)
            if (!std::isfinite(th->weight[c][j])) {
                std::snprintf(msg, sizeof msg, "disk thermal weight[%d][%d] = %.17g is not finite", c, j, th->weight[c][j]);
                return fail(BHG_E_INVALID, msg);
            }
    if (!(std::isfinite(th->t_peak) && th->t_peak > 0.0)) {
        std::snprintf(msg, sizeof msg, "disk thermal t_peak = %.17g must be finite and > 0", th->t_peak);
        return fail(BHG_E_INVALID, msg);
    }
    if (!(std::isfinite(th->f_col) && th->f_col > 0.0)) {
        std::snprintf(msg, sizeof msg, "disk thermal f_col = %.17g must be finite and > 0", th->f_col);
        return fail(BHG_E_INVALID, msg);
    }
    if (!std::isfinite(th->scale)) {
        std::snprintf(msg, sizeof msg, "disk thermal scale = %.17g is not finite", th->scale);
        return fail(BHG_E_INVALID, msg);
    }
    return BHG_OK;
}

// Redshift settings against the trace parameters (include/bhgeo.h, "redshift"): *out = the kernels' parameters.  disk_r_in
// < 0: no disk to check (none in the scene, or the disk class is not asked for).  Also used by bhgeo_frame.hip.
int redshift_params(const bhg_params *p, const bhg_redshift *rs, double disk_r_in, const double *x0, RedshiftParams *out)
{
    BHG_TRY(validate(p));
    if (!rs) return fail(BHG_E_INVALID, "redshift settings are NULL");
    if (rs->apply & ~(BHG_REDSHIFT_DISK | BHG_REDSHIFT_OBJECTS | BHG_REDSHIFT_SKY))
        return fail(BHG_E_INVALID, "redshift apply has bits outside BHG_REDSHIFT_DISK | _OBJECTS | _SKY: " + std::to_string(rs->apply));
    if (!std::isfinite(rs->exponent)) return fail(BHG_E_INVALID, "redshift exponent is not finite");
    if (p->time_like) return fail(BHG_E_INVALID, "redshift is defined for null rays: time_like = 1 is refused");
    if (rs->disk_sense != 1 && rs->disk_sense != -1)
        return fail(BHG_E_INVALID, "redshift disk_sense must be +1 or -1, not " + std::to_string(rs->disk_sense));
    // (s: the sense the formulas use, the traced picture's -- the received photon runs the traced curve mirrored in phi)
    const double M = 0.5 * p->r_s, a = p->rhs_form == BHG_RHS_KERR_BL ? p->spin : 0.0, s = -(double)rs->disk_sense;
    if (disk_r_in >= 0.0) {
        // no timelike circular orbit at or inside the circular photon orbit of this sense (Boyer-Lindquist r)
        const double r_ph = p->rhs_form == BHG_RHS_KERR_BL ? 2.0 * M * (1.0 + std::cos(2.0 / 3.0 * std::acos(-s * a / M))) : 3.0 * M;
        const double r_in = std::sqrt(std::max(disk_r_in * disk_r_in - a * a, 0.0));
        if (!(r_in > r_ph)) {
            char msg[200];
            std::snprintf(msg, sizeof msg, "redshift: disk_r_in %.17g (Boyer-Lindquist r %.17g) is at or inside the circular photon orbit "
                          "r_ph = %.17g of disk_sense %d: no timelike circular orbit there", disk_r_in, r_in, r_ph, rs->disk_sense);
            return fail(BHG_E_INVALID, msg);
        }
    }
    if (x0 && !(std::isfinite(x0[0]) && std::isfinite(x0[1]) && std::isfinite(x0[2])))
        return fail(BHG_E_INVALID, "camera origin is not finite");
    std::memset(out, 0, sizeof(*out));
    if (x0) std::memcpy(out->x0, x0, sizeof(out->x0));
    out->r_s = p->r_s;
    out->spin = a;
    out->sense = (double)rs->disk_sense;
    out->exponent = rs->exponent;
    out->rhs = p->rhs_form;
    out->apply = rs->apply;
    return BHG_OK;
}

// A camera position a ZAMO tetrad exists at (include/bhgeo.h, "the observer camera"): finite, outside the horizon, and for Kerr
// outside the ergosurface and off the BL axis.  who: the messages' prefix.  Used by the observer and polarisation checks.
int camera_position_check(const bhg_params *p, const double *x0, const char *who)
{
    if (!(std::isfinite(x0[0]) && std::isfinite(x0[1]) && std::isfinite(x0[2])))
        return fail(BHG_E_INVALID, "camera origin is not finite");
    const double M = 0.5 * p->r_s;
    char msg[256];
    if (p->rhs_form == BHG_RHS_KERR_BL) {
        const double a = p->spin, rho2 = x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2], bb = rho2 - a * a;
        const double r = std::sqrt(0.5 * (bb + std::sqrt(bb * bb + 4.0 * a * a * x0[2] * x0[2])));
        const double r_plus = M + std::sqrt(M * M - a * a);
        if (!(r > r_plus)) {
            std::snprintf(msg, sizeof msg, "%s: the camera's Boyer-Lindquist r = %.17g is at or inside the horizon r_+ = %.17g",
                          who, r, r_plus);
            return fail(BHG_E_INVALID, msg);
        }
        // inside the ergoregion g_tt > 0: the start conversion's root of the null condition (the one the trace and the
        // redshift take k^t from) is no longer the tetrad's future-directed one, so the trace would follow another photon
        const double c = x0[2] / r, r_ergo = M + std::sqrt(M * M - a * a * c * c);
        if (!(r > r_ergo)) {
            std::snprintf(msg, sizeof msg, "%s: the camera's Boyer-Lindquist r = %.17g is at or inside the ergosurface "
                          "r_E(theta) = %.17g (cos theta = %.17g)", who, r, r_ergo, c);
            return fail(BHG_E_INVALID, msg);
        }
        if (x0[0] == 0.0 && x0[1] == 0.0) {
            std::snprintf(msg, sizeof msg, "%s: a Kerr camera exactly on the axis (x = y = 0) has no azimuthal tetrad leg", who);
            return fail(BHG_E_INVALID, msg);
        }
    } else {
        const double r = std::sqrt(x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2]);
        if (!(r > p->r_s)) {
            std::snprintf(msg, sizeof msg, "%s: the camera's r = %.17g is at or inside the horizon r_s = %.17g", who, r, p->r_s);
            return fail(BHG_E_INVALID, msg);
        }
    }
    return BHG_OK;
}

// Observer settings against the trace parameters and the camera (include/bhgeo.h, "the observer camera"): *out = the
// kernels' parameters, on = 1.  x0 may be NULL (per-ray origins: nothing to check the position of).  Also used by
// bhgeo_frame.hip.
int observer_params(const bhg_params *p, const bhg_observer *obs, const double *x0, ObserverParams *out)
{
    BHG_TRY(validate(p));
    if (!obs) return fail(BHG_E_INVALID, "observer is NULL");
    const double *b = obs->beta;
    if (!(std::isfinite(b[0]) && std::isfinite(b[1]) && std::isfinite(b[2])))
        return fail(BHG_E_INVALID, "observer beta is not finite");
    const double b2 = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
    if (!(b2 < 1.0)) {
        char msg[160];
        std::snprintf(msg, sizeof msg, "observer: |beta| = %.17g must be < 1", std::sqrt(b2));
        return fail(BHG_E_INVALID, msg);
    }
    if (p->time_like) return fail(BHG_E_INVALID, "the observer camera makes null rays: time_like = 1 is refused");
    std::memset(out, 0, sizeof(*out));
    if (x0) {
        BHG_TRY(camera_position_check(p, x0, "observer"));
        std::memcpy(out->x0, x0, sizeof(out->x0));
    }
    std::memcpy(out->beta, b, sizeof(out->beta));
    out->r_s = p->r_s;
    out->spin = p->rhs_form == BHG_RHS_KERR_BL ? p->spin : 0.0;
    out->rhs = p->rhs_form;
    out->on = 1;
    return BHG_OK;
}

// Polarisation settings (include/bhgeo.h, "disk polarisation"): *out = the kernels' parameters, on = 1.  disk_r_in < 0: no
// disk to check; rs: the redshift settings of the same call or NULL; obs: the observer or NULL; x0: the shared camera, or NULL
// (per-ray origins: nothing to check the position of).
int polarisation_params(const bhg_params *p, const bhg_polarisation *pol, const bhg_redshift *rs, const bhg_observer *obs,
                        double disk_r_in, const double *x0, PolarisationParams *out)
{
    BHG_TRY(validate(p));
    if (!pol) return fail(BHG_E_INVALID, "polarisation settings are NULL");
    if (pol->disk_sense != 1 && pol->disk_sense != -1)
        return fail(BHG_E_INVALID, "polarisation disk_sense must be +1 or -1, not " + std::to_string(pol->disk_sense));
    if (pol->n_degree < 1 || pol->n_degree > BHG_POL_TABLE_MAX)
        return fail(BHG_E_INVALID, "polarisation n_degree must be in [1, 64], not " + std::to_string(pol->n_degree));
    for (int j = 0; j < pol->n_degree; j++)
        if (!(std::isfinite(pol->degree[j]) && pol->degree[j] >= 0.0 && pol->degree[j] <= 1.0)) {
            char msg[160];
            std::snprintf(msg, sizeof msg, "polarisation degree[%d] = %.17g must be finite and in [0, 1]", j, pol->degree[j]);
            return fail(BHG_E_INVALID, msg);
        }
    const double *u = pol->up;
    if (!(std::isfinite(u[0]) && std::isfinite(u[1]) && std::isfinite(u[2])) || (u[0] == 0.0 && u[1] == 0.0 && u[2] == 0.0))
        return fail(BHG_E_INVALID, "polarisation up must be finite and not zero");
    if (p->time_like) return fail(BHG_E_INVALID, "polarisation is defined for null rays: time_like = 1 is refused");
    const double M = 0.5 * p->r_s, a = p->rhs_form == BHG_RHS_KERR_BL ? p->spin : 0.0, s = -(double)pol->disk_sense;
    if (disk_r_in >= 0.0) {
        // section 9's rule: no timelike circular orbit at or inside the photon orbit of the traced picture's sense
        const double r_ph = p->rhs_form == BHG_RHS_KERR_BL ? 2.0 * M * (1.0 + std::cos(2.0 / 3.0 * std::acos(-s * a / M))) : 3.0 * M;
        const double r_in = std::sqrt(std::max(disk_r_in * disk_r_in - a * a, 0.0));
        if (!(r_in > r_ph)) {
            char msg[220];
            std::snprintf(msg, sizeof msg, "polarisation: disk_r_in %.17g (Boyer-Lindquist r %.17g) is at or inside the circular photon "
                          "orbit r_ph = %.17g of disk_sense %d", disk_r_in, r_in, r_ph, pol->disk_sense);
            return fail(BHG_E_INVALID, msg);
        }
    }
    if (rs && rs->disk_sense != pol->disk_sense)
        return fail(BHG_E_INVALID, "polarisation disk_sense " + std::to_string(pol->disk_sense) + " differs from the redshift's " +
                                   std::to_string(rs->disk_sense));
    if (x0) BHG_TRY(camera_position_check(p, x0, "polarisation"));
    std::memset(out, 0, sizeof(*out));
    std::memcpy(out->degree, pol->degree, sizeof(double) * (size_t)pol->n_degree);
    std::memcpy(out->up, pol->up, sizeof(out->up));
    if (x0) std::memcpy(out->x0, x0, sizeof(out->x0));
    if (obs) std::memcpy(out->beta, obs->beta, sizeof(out->beta));
    out->r_s = p->r_s;
    out->spin = a;
    out->sense = (double)pol->disk_sense;
    out->n_degree = pol->n_degree;
    out->rhs = p->rhs_form;
    out->on = 1;
    return BHG_OK;
}

// The Page-Thorne constants of the family a*  into *T: r_ms (Bardeen-Press-Teukolsky, a* signed), x0, the
// roots of x^3 - 3x + 2a*, the c_i (a* = 0: the roots sqrt(3), 0, -sqrt(3) and c_2 = 0, the limit of a term that vanishes),
// and 1 / max F^: a grid over x in (x0, 4 x0] brackets the one maximum, a golden-section search closes in on it (the maximum
// is flat, so F^ there is good to the last bits long before x is).  M = 1: F^ is a function of x and a* alone.
void thermal_constants(double astar, ThermalParams *T)
{
    const double z1 = 1.0 + std::cbrt(1.0 - astar * astar) * (std::cbrt(1.0 + astar) + std::cbrt(1.0 - astar));
    const double z2 = std::sqrt(3.0 * astar * astar + z1 * z1);
    const double r_ms = 3.0 + z2 - (astar < 0.0 ? -1.0 : 1.0) * std::sqrt((3.0 - z1) * (3.0 + z1 + 2.0 * z2));
    T->astar = astar;
    T->r_ms = r_ms;         // (in units of M: the caller scales it)
    T->x0 = std::sqrt(r_ms);
    if (astar == 0.0) {
        T->xr[0] = std::sqrt(3.0);
        T->xr[1] = 0.0;
        T->xr[2] = -std::sqrt(3.0);
    } else {
        const double th = std::acos(astar) / 3.0, pi3 = M_PI / 3.0;
        T->xr[0] = 2.0 * std::cos(th - pi3);
        T->xr[1] = 2.0 * std::cos(th + pi3);
        T->xr[2] = -2.0 * std::cos(th);
    }
    for (int i = 0; i < 3; i++) {
        const double xi = T->xr[i], xj = T->xr[(i + 1) % 3], xk = T->xr[(i + 2) % 3];
        T->c[i] = xi == 0.0 ? 0.0 : 3.0 * (xi - astar) * (xi - astar) / (xi * (xi - xj) * (xi - xk));
    }
    const double x0 = T->x0;
    const int N = 3000;
    int best = 1;
    double fbest = -1.0;
    for (int k = 1; k <= N; k++) {
        const double f = page_thorne(*T, x0 * (1.0 + 3.0 * k / N));
        if (f > fbest) {
            fbest = f;
            best = k;
        }
    }
    double lo = x0 * (1.0 + 3.0 * (best - 1) / N), hi = x0 * (1.0 + 3.0 * (best + 1) / N);
    const double gr = 0.5 * (std::sqrt(5.0) - 1.0);
    double u = hi - gr * (hi - lo), v = lo + gr * (hi - lo), fu = page_thorne(*T, u), fv = page_thorne(*T, v);
    for (int it = 0; it < 200 && hi - lo > 1e-15 * hi; it++) {
        if (fu > fv) {
            hi = v;
            v = u;
            fv = fu;
            u = hi - gr * (hi - lo);
            fu = page_thorne(*T, u);
        } else {
            lo = u;
            u = v;
            fu = fv;
            v = lo + gr * (hi - lo);
            fv = page_thorne(*T, v);
        }
    }
    T->inv_fmax = 1.0 / std::max(std::max(fu, fv), fbest);
}

// Thermal-disk settings (include/bhgeo.h, "the thermal disk"): *out = the kernels' table, on = 1, and *rp = the metric, camera
// and sense of the disk's g (apply 0: the caller puts its redshift's apply and exponent in when it has one).  disk_r_in < 0: no
// disk to check; rs, pol: the redshift and polarisation settings of the same call, or NULL; x0: the shared camera, or NULL
// (per-ray origins: nothing to check the position of).  Also used by bhgeo_frame.hip.
int thermal_params(const bhg_params *p, const bhg_disk_thermal *th, const bhg_redshift *rs, const bhg_polarisation *pol,
                   double disk_r_in, const double *x0, ThermalParams *out, RedshiftParams *rp)
{
    BHG_TRY(validate(p));
    if (!th) return fail(BHG_E_INVALID, "disk thermal settings are NULL");
    BHG_TRY(thermal_check(th));
    if (p->time_like) return fail(BHG_E_INVALID, "the thermal disk is seen by null rays: time_like = 1 is refused");
    const double M = 0.5 * p->r_s, a = p->rhs_form == BHG_RHS_KERR_BL ? p->spin : 0.0, s = -(double)th->disk_sense;
    if (disk_r_in >= 0.0) {
        // section 9's rule: no timelike circular orbit at or inside the photon orbit of the traced picture's sense
        const double r_ph = p->rhs_form == BHG_RHS_KERR_BL ? 2.0 * M * (1.0 + std::cos(2.0 / 3.0 * std::acos(-s * a / M))) : 3.0 * M;
        const double r_in = std::sqrt(std::max(disk_r_in * disk_r_in - a * a, 0.0));
        if (!(r_in > r_ph)) {
            char msg[220];
            std::snprintf(msg, sizeof msg, "disk thermal: disk_r_in %.17g (Boyer-Lindquist r %.17g) is at or inside the circular "
                          "photon orbit r_ph = %.17g of disk_sense %d", disk_r_in, r_in, r_ph, th->disk_sense);
            return fail(BHG_E_INVALID, msg);
        }
    }
    if (rs && rs->disk_sense != th->disk_sense)
        return fail(BHG_E_INVALID, "disk thermal disk_sense " + std::to_string(th->disk_sense) + " differs from the redshift's " +
                                   std::to_string(rs->disk_sense));
    if (pol && pol->disk_sense != th->disk_sense)
        return fail(BHG_E_INVALID, "disk thermal disk_sense " + std::to_string(th->disk_sense) + " differs from the polarisation's " +
                                   std::to_string(pol->disk_sense));
    if (x0) BHG_TRY(camera_position_check(p, x0, "disk thermal"));
    std::memset(out, 0, sizeof(*out));
    thermal_constants(s * a / M, out);
    out->r_ms *= M;
    // nu in units of k_B T_peak / h (h / k_B in K s, exact in the SI)
    const double nu0_inv = 4.799243073366221e-11 / th->t_peak;
    for (int j = 0; j < th->n_nu; j++) {
        out->nu[j] = th->nu[j] * nu0_inv;
        for (int c = 0; c < 3; c++) out->w[c][j] = th->weight[c][j];
    }
    out->t_peak = th->t_peak;
    out->f_col = th->f_col;
    out->scale = th->scale;
    out->n_nu = th->n_nu;
    out->on = 1;
    std::memset(rp, 0, sizeof(*rp));
    if (x0) std::memcpy(rp->x0, x0, sizeof(rp->x0));
    rp->r_s = p->r_s;
    rp->spin = a;
    rp->sense = (double)th->disk_sense;
    rp->rhs = p->rhs_form;
    return BHG_OK;
}

// Object motion on its own (include/bhgeo.h, "moving and spinning object spheres") for a scene of n_spheres spheres: every v and
// w of the slots below n_spheres finite.  Also used by bhgeo_frame.hip.
int motion_check(const bhg_object_motion *mo, int32_t n_spheres)
{
    if (!mo) return fail(BHG_E_INVALID, "object motion is NULL");
    const int n = n_spheres < 0 ? 0 : (n_spheres > BHG_MAX_SPHERES ? BHG_MAX_SPHERES : n_spheres);
    for (int j = 0; j < n; j++)
        for (int q = 0; q < 3; q++)
            if (!std::isfinite(mo->v[j][q]) || !std::isfinite(mo->w[j][q])) {
                char msg[200];
                std::snprintf(msg, sizeof msg, "object motion: sphere %d: v = (%.17g, %.17g, %.17g), w = (%.17g, %.17g, %.17g) must be finite",
                              j, mo->v[j][0], mo->v[j][1], mo->v[j][2], mo->w[j][0], mo->w[j][1], mo->w[j][2]);
                return fail(BHG_E_INVALID, msg);
            }
    return BHG_OK;
}

// Object motion against the spheres {c, rho} [n_spheres][4] and the metric of p (include/bhgeo.h): *out =
// the kernels' table, moving = the spheres with a nonzero v or w, on = (moving != 0).  A moving sphere must stay outside the
// horizon and its motion must be timelike on the whole sphere by the sufficient bounds of section 14.  Also used by
// bhgeo_frame.hip.
int motion_params(const bhg_params *p, const bhg_object_motion *mo, const double *spheres, int32_t n_spheres, MotionParams *out)
{
    BHG_TRY(motion_check(mo, n_spheres));
    BHG_TRY(validate(p));
    std::memset(out, 0, sizeof(*out));
    const int n = n_spheres < 0 ? 0 : (n_spheres > BHG_MAX_SPHERES ? BHG_MAX_SPHERES : n_spheres);
    const bool kerr = p->rhs_form == BHG_RHS_KERR_BL;
    const double M = 0.5 * p->r_s, a = kerr ? p->spin : 0.0, a2 = a * a;
    char msg[320];
    for (int j = 0; j < n; j++) {
        const double *v = mo->v[j], *w = mo->w[j];
        bool zero = true;
        for (int q = 0; q < 3; q++) zero = zero && v[q] == 0.0 && w[q] == 0.0;
        if (zero) continue;
        if (!spheres) return fail(BHG_E_INVALID, "object motion needs the spheres");
        const double *c = spheres + 4 * j, rho = c[3];
        const double cn = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), d = cn - rho;
        const double vn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), wn = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        if (!kerr) {
            if (!(d > p->r_s)) {
                std::snprintf(msg, sizeof msg, "object motion: sphere %d: a moving sphere must lie outside the horizon: |c| - rho = %.17g "
                              "<= r_s = %.17g", j, d, p->r_s);
                return fail(BHG_E_INVALID, msg);
            }
            const double bound = 1.0 - p->r_s / d, speed = vn + wn * rho;
            if (!(speed < bound)) {
                std::snprintf(msg, sizeof msg, "object motion: sphere %d: |v| + |w| rho = %.17g is not < f(|c| - rho) = %.17g: the motion "
                              "is not timelike on the whole sphere by section 14's bound", j, speed, bound);
                return fail(BHG_E_INVALID, msg);
            }
        } else {
            const double r_plus = M + std::sqrt(M * M - a2);
            const double r_lo = d > std::fabs(a) ? std::sqrt(d * d - a2) : 0.0, r_hi = cn + rho;
            if (!(r_lo > r_plus)) {
                std::snprintf(msg, sizeof msg, "object motion: sphere %d: a moving sphere must lie outside the horizon: its Boyer-Lindquist "
                              "r can reach sqrt((|c| - rho)^2 - a^2) = %.17g <= r_+ = %.17g", j, r_lo, r_plus);
                return fail(BHG_E_INVALID, msg);
            }
            // G: sqrt(g_phph) / alpha on the equator, the bound of a rigid rotation's ZAMO-relative speed per unit angular
            // velocity at BL r; F: the bound |V| < F(r) of any velocity (section 14)
            auto G = [&](double r) {
                const double Del = r * r - 2.0 * M * r + a2, R2 = r * r + a2;
                return (R2 * R2 - a2 * Del) / (r * r * std::sqrt(Del));
            };
            const double Del_lo = r_lo * r_lo - 2.0 * M * r_lo + a2, R2_lo = r_lo * r_lo + a2;
            const double F_lo = r_lo * Del_lo / (R2_lo * std::sqrt(R2_lo));
            const double wz = w[2], wp = std::sqrt(w[0] * w[0] + w[1] * w[1]);
            const double D[3] = {v[0] + wz * c[1], v[1] - wz * c[0], v[2]};     // v - w_z z^ x c
            const double Dn = std::sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]) + wp * rho;
            const double beta = std::fabs(wz) * std::max(G(r_lo), G(r_hi)) + Dn / F_lo;
            if (!(beta < 1.0)) {
                std::snprintf(msg, sizeof msg, "object motion: sphere %d: the bound %.17g on the ZAMO-relative speed is not < 1: the "
                              "motion is not timelike on the whole sphere by section 14's bound", j, beta);
                return fail(BHG_E_INVALID, msg);
            }
        }
        std::memcpy(out->v[j], v, sizeof(out->v[j]));
        std::memcpy(out->w[j], w, sizeof(out->w[j]));
        out->moving |= 1u << j;
    }
    out->on = out->moving != 0;
    return BHG_OK;
}

// Object textures (include/bhgeo.h, "textured, oriented and emissive object spheres") for a scene of n_spheres spheres: slots
// at or above n_spheres are not looked at.  *out = the kernels' table (an all-zero rotation becomes the identity), on = 1.
// Also used by bhgeo_frame.hip (there with tex = the host arrays: only whether a slot has one matters).
int object_texture_params(const bhg_object_textures *ot, int32_t n_spheres, ObjectTextureParams *out)
{
    if (!ot) return fail(BHG_E_INVALID, "object textures are NULL");
    std::memset(out, 0, sizeof(*out));
    const int n = n_spheres < 0 ? 0 : (n_spheres > BHG_MAX_SPHERES ? BHG_MAX_SPHERES : n_spheres);
    char msg[256];
    for (int j = 0; j < n; j++) {
        if (ot->mode[j] != BHG_OBJECT_LIT && ot->mode[j] != BHG_OBJECT_EMISSIVE) {
            std::snprintf(msg, sizeof msg, "object textures: sphere %d: mode %d is neither BHG_OBJECT_LIT (0) nor BHG_OBJECT_EMISSIVE (1)",
                          j, (int)ot->mode[j]);
            return fail(BHG_E_INVALID, msg);
        }
        if (!(std::isfinite(ot->emission[j]) && ot->emission[j] >= 0.0)) {
            std::snprintf(msg, sizeof msg, "object textures: sphere %d: emission %.17g must be finite and >= 0", j, ot->emission[j]);
            return fail(BHG_E_INVALID, msg);
        }
        if (ot->tex[j] && (ot->tex_w[j] < 1 || ot->tex_h[j] < 1)) {
            std::snprintf(msg, sizeof msg, "object textures: sphere %d: texture size %d x %d must be at least 1 x 1", j,
                          (int)ot->tex_w[j], (int)ot->tex_h[j]);
            return fail(BHG_E_INVALID, msg);
        }
        const double *R = ot->rot[j];
        bool zero = true, finite = true;
        for (int q = 0; q < 9; q++) {
            zero = zero && R[q] == 0.0;
            finite = finite && std::isfinite(R[q]);
        }
        if (zero) {
            static const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            std::memcpy(out->rot[j], eye, sizeof(eye));
        } else {
            // |R^T R - I| <= 1e-9 element by element, and det R = +1 (an orthonormal R has det +-1)
            double dev = finite ? 0.0 : INFINITY;
            for (int u = 0; u < 3 && finite; u++)
                for (int v = 0; v < 3; v++) {
                    const double rtr = R[u] * R[v] + R[3 + u] * R[3 + v] + R[6 + u] * R[6 + v];
                    dev = std::fmax(dev, std::fabs(rtr - (u == v ? 1.0 : 0.0)));
                }
            const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
                               R[2] * (R[3] * R[7] - R[4] * R[6]);
            if (!(dev <= 1e-9) || !(det > 0.0)) {
                std::snprintf(msg, sizeof msg, "object textures: sphere %d: rotation is neither all zero nor a proper rotation "
                              "(max |R^T R - I| = %.3g, det = %.17g)", j, dev, det);
                return fail(BHG_E_INVALID, msg);
            }
            std::memcpy(out->rot[j], R, sizeof(out->rot[j]));
        }
        out->tex[j] = ot->tex[j];
        out->tex_w[j] = ot->tex[j] ? ot->tex_w[j] : 0;
        out->tex_h[j] = ot->tex[j] ? ot->tex_h[j] : 0;
        out->mode[j] = ot->mode[j];
        out->emission[j] = ot->emission[j];
    }
    out->on = 1;
    return BHG_OK;
}

// A mesh material (include/bhgeo.h, "mesh material") for a mesh of nt triangles.  host_arrays: tri_uv and tri_tex are host
// arrays and are scanned (bhg_frame_set_mesh); otherwise only the struct's own fields are looked at.  Also used by
// bhgeo_frame.hip.
int mesh_material_check(const bhg_mesh_material *m, size_t nt, bool host_arrays)
{
    if (!m) return fail(BHG_E_INVALID, "mesh material is NULL");
    char msg[256];
    if (!(std::isfinite(m->emission) && m->emission >= 0.0)) {
        std::snprintf(msg, sizeof msg, "mesh material: emission %.17g must be finite and >= 0", m->emission);
        return fail(BHG_E_INVALID, msg);
    }
    if (m->n_tex < 0 || m->n_tex > BHG_MESH_TEXTURES_MAX) {
        std::snprintf(msg, sizeof msg, "mesh material: n_tex %d must be in [0, BHG_MESH_TEXTURES_MAX]", (int)m->n_tex);
        return fail(BHG_E_INVALID, msg);
    }
    for (int j = 0; j < m->n_tex; j++)
        if (!m->tex[j] || m->tex_w[j] < 1 || m->tex_h[j] < 1) {
            std::snprintf(msg, sizeof msg, "mesh material: tex[%d] must be an image of at least 1 x 1 (tex_w %d, tex_h %d%s)", j,
                          (int)m->tex_w[j], (int)m->tex_h[j], m->tex[j] ? "" : ", NULL image");
            return fail(BHG_E_INVALID, msg);
        }
    if (m->tri_uv && m->n_tex == 0) return fail(BHG_E_INVALID, "mesh material: tri_uv is given but n_tex is 0");
    if (!host_arrays) return BHG_OK;
    if (m->tri_uv)
        for (size_t i = 0; i < nt * 6; i++)
            if (!(std::fabs((double)m->tri_uv[i]) <= 1048576.0)) {   // (NaN fails the comparison too)
                std::snprintf(msg, sizeof msg, "mesh material: tri_uv of triangle %zu is not finite or beyond 2^20 in magnitude", i / 6);
                return fail(BHG_E_INVALID, msg);
            }
    if (m->tri_tex)
        for (size_t i = 0; i < nt; i++)
            if (m->tri_tex[i] >= m->n_tex) {
                std::snprintf(msg, sizeof msg, "mesh material: tri_tex[%zu] = %d is not below n_tex = %d", i, (int)m->tri_tex[i],
                              (int)m->n_tex);
                return fail(BHG_E_INVALID, msg);
            }
    return BHG_OK;
}
}  // namespace bhg

extern "C" {

int bhg_version(void) { return BHG_ABI_VERSION; }

int bhg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char *bhg_last_error(void) { return g_err.c_str(); }

// the binder's handshake: struct sizes as THIS build of the library lays them out
size_t bhg_params_size(void) { return sizeof(bhg_params); }
size_t bhg_camera_size(void) { return sizeof(bhg_camera); }
size_t bhg_scene_size(void) { return sizeof(bhg_scene); }
size_t bhg_frame_scene_size(void) { return sizeof(bhg_frame_scene); }
size_t bhg_redshift_size(void) { return sizeof(bhg_redshift); }
size_t bhg_observer_size(void) { return sizeof(bhg_observer); }
size_t bhg_object_textures_size(void) { return sizeof(bhg_object_textures); }
size_t bhg_polarisation_size(void) { return sizeof(bhg_polarisation); }
size_t bhg_disk_thermal_size(void) { return sizeof(bhg_disk_thermal); }
size_t bhg_object_motion_size(void) { return sizeof(bhg_object_motion); }
size_t bhg_disk_layers_size(void) { return sizeof(bhg_disk_layers); }
size_t bhg_mesh_material_size(void) { return sizeof(bhg_mesh_material); }

int bhg_abi_check(int abi_version, size_t params_size, size_t camera_size, size_t scene_size, size_t frame_scene_size)
{
    // (a binding written for an older ABI whose every entry point and struct layout this library still has is served:
    // BHG_ABI_COMPAT_MIN .. BHG_ABI_VERSION)
    if (abi_version < BHG_ABI_COMPAT_MIN || abi_version > BHG_ABI_VERSION)
        return fail(BHG_E_INVALID, "ABI mismatch: the binding was written for ABI " + std::to_string(abi_version) + ", this libbhgeo.so is ABI " +
                                       std::to_string(BHG_ABI_VERSION) + " and serves bindings from ABI " + std::to_string(BHG_ABI_COMPAT_MIN) +
                                       " on (include/bhgeo.h)");
    const struct {
        const char *name;
        size_t theirs, ours;
    } t[] = {{"bhg_params", params_size, sizeof(bhg_params)},
             {"bhg_camera", camera_size, sizeof(bhg_camera)},
             {"bhg_scene", scene_size, sizeof(bhg_scene)},
             {"bhg_frame_scene", frame_scene_size, sizeof(bhg_frame_scene)}};
    for (const auto &e : t)
        if (e.theirs != 0 && e.theirs != e.ours)   // (0: the binding does not declare that struct)
            return fail(BHG_E_INVALID, std::string("ABI mismatch: the binding's ") + e.name + " is " + std::to_string(e.theirs) +
                                           " bytes, the library's is " + std::to_string(e.ours) + " (include/bhgeo.h, ABI " +
                                           std::to_string(BHG_ABI_VERSION) + ")");
    return BHG_OK;
}

int bhg_default_params_sized(bhg_params *p, size_t params_size)
{
    if (!p) return fail(BHG_E_INVALID, "params is NULL");
    if (params_size != sizeof(bhg_params))
        return fail(BHG_E_INVALID, "ABI mismatch: the caller's bhg_params is " + std::to_string(params_size) + " bytes, the library's is " +
                                       std::to_string(sizeof(bhg_params)) + " -- nothing was written");
    bhg_default_params(p);
    return BHG_OK;
}

void bhg_default_params(bhg_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->r_s = 1.0;  // mass 0.5 (RelativisticRenderEngine.py:506), r_s = 2 M (:95)
    p->lambda_end = 50.0;  // integration_depth default (:508)
    p->max_step = INFINITY;  // max_integration_step -1 -> inf (:59-60); property default 1e4 (:507)
    p->rtol = 1e-3;  // scipy rk.py:86
    p->atol = 1e-6;
    p->h_fixed = 0.1;
    p->r_exit = 0.0;
    p->method = BHG_METHOD_DP54;
    p->rhs_form = BHG_RHS_CHRISTOFFEL;
    p->max_steps = 0;
    p->order_blocks = 0;
    p->disk_r_in = 0.0;
    p->disk_r_out = 0.0;  // no disk
    p->spin = 0.0;
    p->time_like = 0;
}

int bhg_create(int device, bhg_context **out)
{
    if (!out) return fail(BHG_E_INVALID, "out is NULL");
    *out = nullptr;
    int n = bhg_device_count();
    if (n <= 0) return fail(BHG_E_NO_DEVICE, "no HIP device visible (libbhgeo has no CPU fallback)");
    if (device < 0 || device >= n) return fail(BHG_E_NO_DEVICE, "device index out of range");
    ENTER_DEVICE(device);
    bhg_context *c = new (std::nothrow) bhg_context();
    if (!c) return fail(BHG_E_NOMEM, "host allocation failed");
    c->device = device;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) {
        delete c;
        return fail_hip(e, "hipGetDeviceProperties");
    }
    c->num_cus = prop.multiProcessorCount;
    std::snprintf(c->name, sizeof(c->name), "%s (%s)", prop.name, prop.gcnArchName);
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail_hip(e, "hipStreamCreate");
    }
    e = hipMalloc((void **)&c->counter, 2 * 8 * 256);
    if (e != hipSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return fail_hip(e, "hipMalloc(counter)");
    }
    *out = c;
    return BHG_OK;
}

void bhg_destroy(bhg_context *c)
{
    if (!c) return;
    DeviceGuard guard(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->d_in) (void)hipFree(c->d_in);
    if (c->d_out) (void)hipFree(c->d_out);
    if (c->d_ws) (void)hipFree(c->d_ws);
    if (c->d_endws) (void)hipFree(c->d_endws);
    if (c->pin_in) (void)hipHostFree(c->pin_in);
    if (c->pin_out) (void)hipHostFree(c->pin_out);
    for (int i = 0; i < 2; i++) {
        if (c->ev_in[i]) (void)hipEventDestroy(c->ev_in[i]);
        if (c->ev_k[i]) (void)hipEventDestroy(c->ev_k[i]);
        if (c->ev_out[i]) (void)hipEventDestroy(c->ev_out[i]);
    }
    if (c->s_in) (void)hipStreamDestroy(c->s_in);
    if (c->s_out) (void)hipStreamDestroy(c->s_out);
    if (c->counter) (void)hipFree(c->counter);
    if (c->ev_order) (void)hipEventDestroy(c->ev_order);
    for (int i = 0; i < 4; i++)
        if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bhg_device_name(bhg_context *c, char *buf, size_t buflen)
{
    if (!c || !buf || buflen == 0) return fail(BHG_E_INVALID, "bad argument");
    std::snprintf(buf, buflen, "%s", c->name);
    return BHG_OK;
}

int bhg_num_cus(bhg_context *c) { return c ? c->num_cus : fail(BHG_E_INVALID, "ctx is NULL"); }

int bhg_synchronize(bhg_context *c)
{
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    ENTER_DEVICE(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BHG_OK;
}

int bhg_set_profiling(bhg_context *c, int enable)
{
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    ENTER_DEVICE(c->device);
    if (enable && !c->ev[0])
        for (int i = 0; i < 4; i++) HIP_TRY(hipEventCreate(&c->ev[i]));
    c->profiling = enable != 0;
    c->ev_valid = false;
    return BHG_OK;
}

int bhg_last_pass_ms(bhg_context *c, float out_ms[3])
{
    if (!c || !out_ms) return fail(BHG_E_INVALID, "bad argument");
    if (!c->ev_valid) return fail(BHG_E_INVALID, "no profiled trace call yet (bhg_set_profiling)");
    ENTER_DEVICE(c->device);
    HIP_TRY(hipEventSynchronize(c->ev[c->ev_post ? 3 : 2]));
    for (int i = 0; i < 2; i++) HIP_TRY(hipEventElapsedTime(&out_ms[i], c->ev[i], c->ev[i + 1]));
    // third slot: the pass AFTER the trace kernel -- Kerr's Boyer-Lindquist -> Cartesian finalize (0 for the
    // Schwarzschild forms: events are resolved inside the trace kernel, there is no pass after it)
    out_ms[2] = 0.0f;
    if (c->ev_post) HIP_TRY(hipEventElapsedTime(&out_ms[2], c->ev[2], c->ev[3]));
    return BHG_OK;
}

void *bhg_context_stream(bhg_context *c) { return c ? (void *)c->stream : nullptr; }

int bhg_last_launch(bhg_context *c, int32_t out[4])
{
    if (!c || !out) return fail(BHG_E_INVALID, "bad argument");
    std::memcpy(out, c->last_launch, sizeof(c->last_launch));
    return BHG_OK;
}

}  // extern "C"

namespace {

int validate_spheres(const bhg_params *p, const double *spheres, int32_t n_spheres)
{
    if (n_spheres < 0 || n_spheres > BHG_MAX_SPHERES) return fail(BHG_E_INVALID, "n_spheres must be in [0, BHG_MAX_SPHERES]");
    if (n_spheres == 0) return BHG_OK;
    if (!spheres) return fail(BHG_E_INVALID, "spheres is NULL");
    for (int j = 0; j < n_spheres; j++) {
        const double *sp = spheres + 4 * j;
        if (!std::isfinite(sp[0]) || !std::isfinite(sp[1]) || !std::isfinite(sp[2]) || !std::isfinite(sp[3]) || !(sp[3] > 0.0))
            return fail(BHG_E_INVALID, "sphere centres must be finite and radii finite and > 0");
    }
    return BHG_OK;
}

using bhg::TraceCall;
using bhg::TraceKind;

// ONE launch: tc.n <= BHG_MAX_RAYS_PER_LAUNCH rays (the kernels form a ray's byte offsets in 32 bits).
// tc.kind other than PERSISTENT: a lane-per-ray kernel instead of the persistent one (the caller has checked what that kernel
// does not cover)
int trace_device_one(bhg_context *c, const bhg_params *p, const TraceCall &tc)
{
    const double *const spheres = tc.spheres, *const x0_shared = tc.x0_shared, *const d_x0 = tc.d_x0, *const d_k0 = tc.d_k0;
    const int32_t n_spheres = tc.n_spheres, start_mode = tc.start_mode;
    const size_t n = tc.n;
    double *d_end = tc.d_end, *d_end_dir = tc.d_end_dir;
    uint8_t *const d_flags = tc.d_flags;
    uint32_t *const d_n_steps = tc.d_n_steps, *const d_n_accepted = tc.d_n_accepted;
    bhg_prefix *const pf = tc.prefix;
    const bool lanes = tc.kind != TraceKind::PERSISTENT;
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    BHG_TRY(validate(p));
    BHG_TRY(validate_spheres(p, spheres, n_spheres));
    if (pf) {
        pf->used = BHG_PREFIX_NONE;
        if (pf->mode != BHG_PREFIX_NONE && pf->mode != BHG_PREFIX_RECORD && pf->mode != BHG_PREFIX_REPLAY &&
            pf->mode != BHG_PREFIX_RECORD_DEEP && pf->mode != BHG_PREFIX_RECORD_WIDE && pf->mode != BHG_PREFIX_RECORD_RIM)
            return fail(BHG_E_INVALID,
                        "prefix mode must be BHG_PREFIX_NONE, BHG_PREFIX_RECORD, BHG_PREFIX_REPLAY, BHG_PREFIX_RECORD_DEEP, BHG_PREFIX_RECORD_WIDE "
                        "or BHG_PREFIX_RECORD_RIM");
        if (n && pf->mode != BHG_PREFIX_NONE && !pf->d_records) return fail(BHG_E_INVALID, "prefix mode asks for d_records, which is NULL");
    }
    if (start_mode != BHG_START_NONE && start_mode != BHG_START_RECORD && start_mode != BHG_START_REPLAY)
        return fail(BHG_E_INVALID, "start_mode must be BHG_START_NONE, BHG_START_RECORD or BHG_START_REPLAY");
    if (n == 0) return BHG_OK;
    if (start_mode != BHG_START_NONE && !tc.d_start_steps) return fail(BHG_E_INVALID, "start_mode asks for d_start_steps, which is NULL");
    if (!d_k0 || (!d_end && !d_end_dir)) return fail(BHG_E_INVALID, "k0 / end is NULL");
    if (!x0_shared && !d_x0) return fail(BHG_E_INVALID, "neither x0_shared nor d_x0 given");
    if (n > bhg::BHG_MAX_RAYS_PER_LAUNCH) return fail(BHG_E_INVALID, "internal: more rays than one launch takes");
    ENTER_DEVICE(c->device);
    hipStream_t s = (hipStream_t)tc.stream;
    // Launches of one context share its work counters (launch K zeroes the set launch K + 1 counts on) and its workspace:
    // they must execute in the order they were issued.  On ONE stream they do; a call that arrives on ANOTHER stream than
    // the previous one is ordered behind it here (an event on the old stream, a wait on the new one) -- it then cannot
    // overlap the previous call, but it cannot corrupt it either (two traces that are to overlap need two contexts).
    // The previous call's stream may be a handle the CALLER owns -- and may have destroyed since: it is never touched
    // again.  A call on a caller's stream leaves an event behind it at its own end (below, ev_order recorded on that stream
    // while the caller is still inside the call); only the context's own stream and the null stream, which cannot go away,
    // are recorded on after the fact.
    if (c->launched && s != c->last_stream) {
        if (!c->ev_order) HIP_TRY(hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming));
        if (!c->last_stream_foreign) HIP_TRY(hipEventRecord(c->ev_order, c->last_stream));
        HIP_TRY(hipStreamWaitEvent(s, c->ev_order, 0));
    }
    c->last_stream = s;
    c->launched = true;

    // Workspace, grown on demand (the first call at a new size allocates; steady-state calls do not; the trace kernels work
    // their start records out themselves and parked steps live in the waves' LDS pools, so there are no per-ray records):
    //   flags   [n] bytes       when the caller does not want flags
    //   n_steps / n_accepted [n] u32 when the caller does not want them (the kernels never test these pointers)
    const bool has_exit = p->r_exit > 0.0;
    const bool kerr = p->rhs_form == BHG_RHS_KERR_BL;
    const size_t sz_flags = d_flags ? 0 : ((n + 7) & ~size_t(7));
    const size_t sz_u32 = n * sizeof(uint32_t);
    const size_t sz_steps = !d_n_steps ? sz_u32 : 0;
    const size_t sz_acc = !d_n_accepted ? sz_u32 : 0;
    BHG_TRY(ensure(&c->d_ws, &c->d_ws_bytes, sz_flags + sz_steps + sz_acc + 64));
    if (!d_end && kerr) {
        // direction-only Kerr call: the end records are workspace (the Boyer-Lindquist states the finalize pass converts),
        // final directions are split off into d_end_dir afterwards
        BHG_TRY(ensure(&c->d_endws, &c->d_endws_bytes, n * 6 * sizeof(double) + 64));
        d_end = (double *)c->d_endws;
    } else if (d_end) {
        d_end_dir = nullptr;
    }
    char *wsb = (char *)c->d_ws;
    uint8_t *w_flags = (uint8_t *)wsb;
    uint32_t *w_steps = (uint32_t *)(wsb + sz_flags);
    uint32_t *w_acc = (uint32_t *)(wsb + sz_flags + sz_steps);

    bhg::TraceArgs a;
    std::memset(&a, 0, sizeof(a));
    a.k0 = d_k0;
    a.x0 = d_x0;
    a.end = d_end;
    // (Kerr end states are converted from Boyer-Lindquist by a pass over whole records: directions are split off after it)
    a.end_dir = kerr ? nullptr : d_end_dir;
    a.flags = d_flags ? d_flags : w_flags;
    a.n_steps = d_n_steps ? d_n_steps : w_steps;
    a.n_accepted = d_n_accepted ? d_n_accepted : w_acc;
    a.counter = c->counter + (size_t)c->counter_set * (8 * 256 / sizeof(unsigned long long));
    a.counter_next = c->counter + (size_t)(c->counter_set ^ 1) * (8 * 256 / sizeof(unsigned long long));
    a.n = n;
    if (!d_x0) {
        a.x0s[0] = x0_shared[0];
        a.x0s[1] = x0_shared[1];
        a.x0s[2] = x0_shared[2];
    }
    const int rhs_id = fill_trace_args(a, p, spheres, n_spheres);
    a.min_step_cap = 40.0 * std::nextafter(std::fmax(p->lambda_end, 1.0), INFINITY) * 2.220446049250313e-16;
    // (lambda_end = 0: every ray is "already at t_bound" at its first step -- the rare-path prologue handles that, and an
    // infinite cap sends every lane there)
    if (p->lambda_end == 0.0) a.min_step_cap = INFINITY;
    // work-order hint: honoured when the call is that many equal blocks of whole 64-ray batches
    bool order_hint = p->order_blocks > 1 && n % p->order_blocks == 0 && (n / p->order_blocks) % 64 == 0;
#ifdef BHG_TUNING
    if (std::getenv("BHGEO_NO_ORDER_HINT")) order_hint = false;  // A/B aid, tuning builds only
#endif
    if (order_hint) {
        a.order_blocks = (int32_t)p->order_blocks;
        a.order_block_len = n / p->order_blocks;
    }
    a.object_id = tc.d_object_id;
    // the rays' initial steps kept by their owner (the DP5(4) kernels' queue fill; RK4 has none and never looks)
    a.start_h = start_mode != BHG_START_NONE ? tc.d_start_steps : nullptr;
    a.start_mode = start_mode;
    // the rays' start-up records kept by their owner: shared-origin calls of DP5(4) with the two Cartesian null forms, one launch
    // (the planes' stride is the launch's n), a step budget the records cannot exhaust.  Anything else ignores them, as RK4
    // ignores the start steps, and says so in pf->used.
    bool pf_record = false, pf_deep = false;
    uint32_t pf_acc_max = (uint32_t)BHG_PREFIX_DEEP_ACCEPTED, pf_att_max = (uint32_t)BHG_PREFIX_DEEP_ATTEMPTS;
    double pf_rho = 0.0;
    if (pf && pf->mode != BHG_PREFIX_NONE && !lanes && !d_x0 && p->method == BHG_METHOD_DP54 &&
        (rhs_id == bhg::BHG_RHS_CHRISTOFFEL_ || rhs_id == bhg::BHG_RHS_REDUCED_) && a.max_steps > (uint32_t)BHG_PREFIX_K_MAX) {
        const double clear = bhg::prefix_clearance(a.r_hor, a.r_exit, a.disk_r_out > 0.0, spheres, n_spheres, x0_shared);
        // (a deep record holds up to BHG_PREFIX_DEEP_ATTEMPTS attempts: neither written nor -- the call cannot tell which rule
        // wrote the records it is handed -- replayed under a step budget that those attempts would exhaust)
        const bool deep_fits = a.max_steps > (uint32_t)BHG_PREFIX_DEEP_ATTEMPTS;
        if (pf->mode == BHG_PREFIX_RECORD) {
            pf_rho = bhg::prefix_rho(clear, x0_shared);
            pf_record = pf_rho > 0.0;
        } else if (pf->mode == BHG_PREFIX_RECORD_DEEP) {
            pf_rho = deep_fits ? bhg::prefix_rho_deep_call(clear, a.r_hor, x0_shared, n_spheres) : 0.0;
            pf_record = pf_deep = pf_rho > 0.0;
        } else if (pf->mode == BHG_PREFIX_RECORD_WIDE) {
            // (the deep recorder in the wider ball, with room for the accepted steps that ball holds; where the rule keeps the
            // deep call's ball it keeps its cap, and the records are that call's byte for byte)
            pf_rho = deep_fits ? bhg::prefix_rho_wide_call(clear, a.r_hor, x0_shared, n_spheres) : 0.0;
            pf_record = pf_deep = pf_rho > 0.0;
            if (pf_rho > bhg::prefix_rho_deep_call(clear, a.r_hor, x0_shared, n_spheres)) pf_acc_max = (uint32_t)BHG_PREFIX_WIDE_ACCEPTED;
        } else if (pf->mode == BHG_PREFIX_RECORD_RIM) {
            // (the same recorder in the ball that ends just above the horizon, with both caps raised to what that ball holds; where
            // the rule keeps the wide call's ball it keeps that call's caps and budget, and the records are that call's byte for byte)
            const double wide_rho = bhg::prefix_rho_wide_call(clear, a.r_hor, x0_shared, n_spheres);
            pf_rho = deep_fits ? bhg::prefix_rho_rim_call(clear, a.r_hor, x0_shared, n_spheres) : 0.0;
            if (pf_rho > wide_rho) {
                pf_acc_max = (uint32_t)BHG_PREFIX_RIM_ACCEPTED;
                pf_att_max = (uint32_t)BHG_PREFIX_RIM_ATTEMPTS;
                if (!(a.max_steps > (uint32_t)BHG_PREFIX_RIM_ATTEMPTS)) pf_rho = 0.0;
            } else if (pf_rho > bhg::prefix_rho_deep_call(clear, a.r_hor, x0_shared, n_spheres)) {
                pf_acc_max = (uint32_t)BHG_PREFIX_WIDE_ACCEPTED;
            }
            pf_record = pf_deep = pf_rho > 0.0;
        } else if (deep_fits && a.max_steps <= (uint32_t)BHG_PREFIX_RIM_ATTEMPTS && bhg::prefix_rho_is_rim(pf->rho, a.r_hor, x0_shared)) {
            // (rim records say so by their rho: from this origin no other rule writes one this large.  They hold up to
            // BHG_PREFIX_RIM_ATTEMPTS attempts, and a caller that asks for them under a budget those would exhaust is told)
            return fail(BHG_E_INVALID, "BHG_PREFIX_REPLAY of rim records needs max_steps > BHG_PREFIX_RIM_ATTEMPTS");
        } else if (deep_fits && bhg::prefix_replay_ok(clear, pf->rho)) {
            a.prefix = (const double2 *)pf->d_records;
            pf->used = BHG_PREFIX_REPLAY;
        }
    }
    // kernel variant: bit 0 exit sphere, bit 1 disk, bit 2 objects.  With objects: 5 = exit sphere and no disk (the
    // orbiting-sphere frames), otherwise 7, which tests for the exit sphere and the disk at run time
    int evt = n_spheres > 0 ? ((has_exit && !(p->disk_r_out > 0.0)) ? 5 : 7)
                            : ((has_exit ? 1 : 0) | (p->disk_r_out > 0.0 ? 2 : 0));
    if (rhs_id == bhg::BHG_RHS_CHRISTOFFEL_TL_) evt = 7;    // (the time-like form exists in the all-events variant only)

    size_t grid = (n + 63) / 64;
    int per_cu = 0;
    if (lanes) {
        // a lane-per-ray trace: no work counters, no resident-wave count
        a.cross = tc.cross;
        a.n_cross = tc.n_cross;
        a.max_cross = tc.max_cross;
        a.cross_stride = tc.stride;
        if (tc.kind == TraceKind::MESH) {
            bhg::MeshArgs g;
            std::memset(&g, 0, sizeof(g));
            g.mesh = tc.mesh->view;
            std::memcpy(g.box, tc.mesh->box, sizeof(g.box));
            g.d_min = tc.mesh->d_min;
            g.d_max = tc.mesh->d_max;
            g.max_chord = tc.max_chord;
            g.cull = bhg::mesh_culls_on();
            g.tri_id = tc.tri_id;
            g.bary = tc.bary;
            if (tc.instances) {
                // the placements: the whole-step cull against their union, the records beside
                const bhg_mesh_instances *in = tc.instances;
                std::memcpy(g.box, in->box, sizeof(g.box));
                g.d_min = in->d_min;
                g.d_max = in->d_max;
                HIP_TRY(bhg::instances_before_read(in, s));
                if (in->leaf_size && bhg::instance_tree_on()) {
                    // a set under a tree: the records and the tree over them
                    bhg::MeshInstanceTreeArgs ta;
                    std::memset(&ta, 0, sizeof(ta));
                    ta.tree = in->tree;
                    ta.inst_id = tc.inst_id;
                    ta.cull = g.cull;
                    HIP_TRY(bhg::launch_trace_mesh_instance_tree(a, g, ta, rhs_id, s));
                } else {
                    // (a set under a tree with BHGEO_INSTANCE_TREE=0 as well: the linear loop has no limit of its own)
                    bhg::MeshInstanceArgs ia;
                    std::memset(&ia, 0, sizeof(ia));
                    ia.rec = in->d_rec;
                    ia.n = in->n;
                    ia.inst_id = tc.inst_id;
                    ia.cull = g.cull;       // (BHGEO_MESH_CULL=0 takes the instances' world boxes out as well)
                    HIP_TRY(bhg::launch_trace_mesh_instances(a, g, ia, rhs_id, s));
                }
                HIP_TRY(bhg::instances_after_read(in, s));
            } else {
                HIP_TRY(bhg::launch_trace_mesh(a, g, rhs_id, s));
            }
        } else if (tc.kind == TraceKind::TRAVEL_TIME) {
            HIP_TRY(bhg::launch_travel_time(a, rhs_id, tc.t_end, tc.t_cross, s));
        } else {
            HIP_TRY(bhg::launch_trace_crossings(a, rhs_id, s));
        }
        c->ev_valid = false;
    } else {
        // resident waves per CU of the trace kernel variant: asked of the runtime once per variant and context
        const int vkey = ((p->method & 1) * 3 + (p->rhs_form % 3)) * 8 + evt + (rhs_id == bhg::BHG_RHS_CHRISTOFFEL_TL_ ? 48 : 0);
        per_cu = c->occupancy[vkey];
        if (per_cu == 0) {
            HIP_TRY(bhg::trace_occupancy(p->method, rhs_id, evt, &per_cu));
            if (per_cu < 1) per_cu = 1;
            if (per_cu > 32) per_cu = 32;
            c->occupancy[vkey] = per_cu;
        }
#ifdef BHG_TUNING
        if (const char *ov = std::getenv("BHGEO_WAVES_PER_CU")) {  // tuning / diagnostic override
            int v = std::atoi(ov);
            if (v >= 1 && v <= 64) per_cu = v;
        }
#endif
        // persistent waves: fill every resident wave slot once; never more waves than 64-ray batches
        size_t batches = (n + 63) / 64;
        grid = (size_t)per_cu * (size_t)c->num_cus;
        if (grid > batches) grid = batches;
#ifdef BHG_DIAG
        {
            static unsigned long long *dbuf = nullptr;
            if (!dbuf) HIP_TRY(hipMalloc((void **)&dbuf, 65536 * 8 * sizeof(unsigned long long)));
            a.diag = dbuf;
            a.dbg_idx = std::getenv("BHGEO_DBG_IDX") ? (uint32_t)std::atoi(std::getenv("BHGEO_DBG_IDX")) : 0xFFFFFFFFu;
            if (const char *path = std::getenv("BHGEO_DIAG_DUMP")) {
                static unsigned long long host[65536 * 8];
                HIP_TRY(hipDeviceSynchronize());
                HIP_TRY(hipMemcpy(host, dbuf, sizeof(host), hipMemcpyDeviceToHost));
                if (FILE *f = std::fopen(path, "wb")) {
                    std::fwrite(host, 1, sizeof(host), f);
                    std::fclose(f);
                }
            }
        }
#endif
        // ONE persistent launch finishes every ray: events are resolved and rays resumed inside the trace kernel, so
        // the call only enqueues (Kerr: trace, finalize) and returns
        if (!c->counters_clean) HIP_TRY(hipMemsetAsync(c->counter, 0, 2 * 8 * 256, s));   // first call, or after a failed enqueue
        if (pf_record) {
            // the recording pass, in front of the trace of always (which starts its rays itself: the records are for later calls)
            HIP_TRY(bhg::launch_record_prefix(a, rhs_id, pf->d_records, pf_rho, pf_deep, pf_acc_max, pf_att_max, s));
            pf->rho = pf_rho;
            pf->used = pf->mode;
        }
        c->counters_clean = false;
        HIP_TRY(bhg::launch_trace(a, p->method, rhs_id, evt, (int)grid, s, c->profiling ? c->ev : nullptr));
        c->counter_set ^= 1;      // (the launch is in the stream: the next call of this context counts on the set it zeroes)
        c->counters_clean = true;
        c->ev_valid = c->profiling;
    }
    c->last_launch[3] = 1;
    c->ev_post = false;
    if (p->rhs_form == BHG_RHS_KERR_BL) {
        // (direction-only calls: the finalize pass writes the Cartesian exit directions straight into d_end_dir)
        HIP_TRY(bhg::launch_kerr_finalize(a, d_end_dir, s));
        if (c->profiling && !lanes) {
            HIP_TRY(hipEventRecord(c->ev[3], s));
            c->ev_post = true;
        }
    }
    c->last_launch[0] = (int32_t)grid;
    c->last_launch[1] = 64;
    c->last_launch[2] = per_cu;
    // a caller's stream: leave the ordering event behind this call now, while the handle is certainly alive (the next
    // call on another stream waits on it and never touches this stream again)
    c->last_stream_foreign = s != nullptr && s != c->stream;
    if (c->last_stream_foreign) {
        if (!c->ev_order) HIP_TRY(hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(c->ev_order, s));
    }
    return BHG_OK;
}

// A trace call of any size: launches of at most BHG_MAX_RAYS_PER_LAUNCH rays, one after the other on the caller's stream
// (BASELINE's largest frame, 2048 x 2048 x 16 = 2^26 rays, is one launch).  Every ray is its own ODE: the split never
// changes a result.  The work-order hint describes ONE launch's rays and is dropped for a split call.
int trace_device_impl(bhg_context *c, const bhg_params *p, const TraceCall &tc)
{
    const size_t n = tc.n;
    if (n <= bhg::BHG_MAX_RAYS_PER_LAUNCH) return trace_device_one(c, p, tc);
    if (tc.prefix) tc.prefix->used = BHG_PREFIX_NONE;    // (a split call: the records' planes are strided by ONE launch's ray count)
    if (!p) return fail(BHG_E_INVALID, "params is NULL");
    if (n > 0xFFFFFFFFull) return fail(BHG_E_INVALID, "n must be < 2^32 per call");
    bhg_params q = *p;
    q.order_blocks = 0;
    BHG_TRY(bhg::for_each_launch(tc, bhg::BHG_MAX_RAYS_PER_LAUNCH, [&](const TraceCall &part) { return trace_device_one(c, &q, part); }));
    c->last_launch[3] = (int32_t)((n + bhg::BHG_MAX_RAYS_PER_LAUNCH - 1) / bhg::BHG_MAX_RAYS_PER_LAUNCH);
    return BHG_OK;
}

// The round trip of a plain host-buffer call on the context's stream.  Every array is named once and gets a region of ONE device
// block (bhg::StageLayout), the call's own or the context's d_in.  run() allocates, uploads, makes the _device call (which takes
// its arrays from at()), downloads and waits; copies go in the order the arrays were named.  However the call ends, the stream is
// drained and a block of the call's own is freed.
class Staged {
public:
    static constexpr size_t NONE = ~size_t(0);   // the place of an array that is not there: at() gives null
    Staged(bhg_context *ctx, bool own_block) : c(ctx), own(own_block) {}
    ~Staged()
    {
        (void)hipStreamSynchronize(c->stream);
        if (own) (void)hipFree(d);
    }
    // an input and an in-out array may be NULL (not there); an output that is NULL is optional: staged, not brought back
    size_t in(const void *host, size_t bytes) { return host ? add(bytes, host, nullptr) : NONE; }
    size_t out(void *host, size_t bytes) { return add(bytes, nullptr, host); }
    size_t inout(void *host, size_t bytes) { return host ? add(bytes, host, host) : NONE; }
    template <class T>
    T *at(size_t off) const { return off == NONE ? nullptr : (T *)(d + off); }
    template <class Call>
    int run(Call &&device_call)
    {
        if (count > MAX) return fail(BHG_E_INVALID, "internal: more staged arrays than a call names");
        if (own) {
            HIP_TRY(hipMalloc((void **)&d, layout.total()));
        } else {
            BHG_TRY(ensure(&c->d_in, &c->d_in_bytes, layout.total()));
            d = (char *)c->d_in;
        }
        for (int i = 0; i < count; i++)
            if (r[i].up) HIP_TRY(hipMemcpyAsync(d + r[i].off, r[i].up, r[i].bytes, hipMemcpyHostToDevice, c->stream));
        BHG_TRY(device_call());
        for (int i = 0; i < count; i++)
            if (r[i].down) HIP_TRY(hipMemcpyAsync(r[i].down, d + r[i].off, r[i].bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return BHG_OK;
    }

private:
    static constexpr int MAX = 12;
    size_t add(size_t bytes, const void *up, void *down)
    {
        const size_t off = layout.add(bytes);
        if (count < MAX) r[count] = {off, bytes, up, down};
        count++;
        return off;
    }
    bhg_context *c;
    bhg::StageLayout layout;
    struct { size_t off, bytes; const void *up; void *down; } r[MAX];
    int count = 0;
    char *d = nullptr;
    bool own;
};

}  // namespace

extern "C" {

int bhg_trace_device(bhg_context *c, const bhg_params *p, const double *x0_shared, const double *d_x0,
                     const double *d_k0, size_t n, double *d_end, uint8_t *d_flags, uint32_t *d_n_steps,
                     uint32_t *d_n_accepted, void *stream)
{
    return trace_device_impl(c, p, {.x0_shared = x0_shared, .d_x0 = d_x0, .d_k0 = d_k0, .n = n, .d_end = d_end, .d_flags = d_flags,
                                    .d_n_steps = d_n_steps, .d_n_accepted = d_n_accepted, .stream = stream});
}

int bhg_trace_dir_device(bhg_context *c, const bhg_params *p, const double *x0_shared, const double *d_x0,
                         const double *d_k0, size_t n, double *d_end_dir, uint8_t *d_flags, uint32_t *d_n_steps,
                         uint32_t *d_n_accepted, void *stream)
{
    if (n && !d_end_dir) return fail(BHG_E_INVALID, "end_dir is NULL");
    return trace_device_impl(c, p, {.x0_shared = x0_shared, .d_x0 = d_x0, .d_k0 = d_k0, .n = n, .d_end_dir = d_end_dir,
                                    .d_flags = d_flags, .d_n_steps = d_n_steps, .d_n_accepted = d_n_accepted, .stream = stream});
}

int bhg_trace_objects_device(bhg_context *c, const bhg_params *p, const double *spheres, int32_t n_spheres,
                             const double *x0_shared, const double *d_x0, const double *d_k0, size_t n, double *d_end,
                             uint8_t *d_flags, uint32_t *d_n_steps, uint32_t *d_n_accepted, int8_t *d_object_id,
                             void *stream)
{
    return trace_device_impl(c, p, {.spheres = spheres, .n_spheres = n_spheres, .x0_shared = x0_shared, .d_x0 = d_x0, .d_k0 = d_k0,
                                    .n = n, .d_end = d_end, .d_flags = d_flags, .d_n_steps = d_n_steps,
                                    .d_n_accepted = d_n_accepted, .d_object_id = d_object_id, .stream = stream});
}

int bhg_trace_start_device(bhg_context *c, const bhg_params *p, const double *spheres, int32_t n_spheres,
                           const double *x0_shared, const double *d_x0, const double *d_k0, size_t n, double *d_end,
                           double *d_end_dir, uint8_t *d_flags, uint32_t *d_n_steps, uint32_t *d_n_accepted,
                           int8_t *d_object_id, double *d_start_steps, int32_t start_mode, void *stream)
{
    if (n && !d_end && !d_end_dir) return fail(BHG_E_INVALID, "end / end_dir is NULL");
    return trace_device_impl(c, p, {.spheres = spheres, .n_spheres = n_spheres, .x0_shared = x0_shared, .d_x0 = d_x0, .d_k0 = d_k0,
                                    .n = n, .d_end = d_end, .d_end_dir = d_end ? nullptr : d_end_dir, .d_flags = d_flags,
                                    .d_n_steps = d_n_steps, .d_n_accepted = d_n_accepted, .d_object_id = d_object_id,
                                    .d_start_steps = d_start_steps, .start_mode = start_mode, .stream = stream});
}

int bhg_trace_prefix_device(bhg_context *c, const bhg_params *p, const double *spheres, int32_t n_spheres,
                            const double *x0_shared, const double *d_x0, const double *d_k0, size_t n, double *d_end,
                            double *d_end_dir, uint8_t *d_flags, uint32_t *d_n_steps, uint32_t *d_n_accepted,
                            int8_t *d_object_id, double *d_start_steps, int32_t start_mode, bhg_prefix *prefix, void *stream)
{
    if (n && !d_end && !d_end_dir) return fail(BHG_E_INVALID, "end / end_dir is NULL");
    if (!prefix) return fail(BHG_E_INVALID, "prefix is NULL");
    return trace_device_impl(c, p, {.spheres = spheres, .n_spheres = n_spheres, .x0_shared = x0_shared, .d_x0 = d_x0, .d_k0 = d_k0,
                                    .n = n, .d_end = d_end, .d_end_dir = d_end ? nullptr : d_end_dir, .d_flags = d_flags,
                                    .d_n_steps = d_n_steps, .d_n_accepted = d_n_accepted, .d_object_id = d_object_id,
                                    .d_start_steps = d_start_steps, .start_mode = start_mode, .prefix = prefix, .stream = stream});
}

double bhg_prefix_clearance(const bhg_params *p, const double *spheres, int32_t n_spheres, const double *x0)
{
    if (!p || !x0 || n_spheres < 0 || (n_spheres > 0 && !spheres)) return 0.0;
    bhg::TraceArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_trace_args(a, p, nullptr, 0);
    return bhg::prefix_clearance(a.r_hor, a.r_exit, a.disk_r_out > 0.0, spheres, n_spheres, x0);
}

int32_t bhg_prefix_deep_attempts(void) { return BHG_PREFIX_DEEP_ATTEMPTS; }
int32_t bhg_prefix_wide_accepted(void) { return BHG_PREFIX_WIDE_ACCEPTED; }
int32_t bhg_prefix_rim_attempts(void) { return BHG_PREFIX_RIM_ATTEMPTS; }

// when an owner records again: bhg::PrefixOwner (prefix_clearance.h) on the call's own clearance, for bhg_frame_render and the binding alike
static_assert(sizeof(bhg_prefix_owner) == 24, "bhg_prefix_owner layout is part of the ABI");
int32_t bhg_prefix_owner_next(bhg_prefix_owner *o, int32_t rule, int32_t promote, const bhg_params *p, const double *spheres,
                              int32_t n_spheres, const double *x0, const bhg_prefix *last)
{
    if (!o || !p || !x0 || n_spheres < 0 || (n_spheres > 0 && !spheres)) return BHG_PREFIX_NONE;
    if (!bhg::prefix_mode_records(rule)) return BHG_PREFIX_NONE;
    if (promote != BHG_PREFIX_NONE && promote != BHG_PREFIX_RECORD_DEEP && promote != BHG_PREFIX_RECORD_WIDE && promote != BHG_PREFIX_RECORD_RIM)
        return BHG_PREFIX_NONE;
    bhg::TraceArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_trace_args(a, p, nullptr, 0);
    const double clear = bhg::prefix_clearance(a.r_hor, a.r_exit, a.disk_r_out > 0.0, spheres, n_spheres, x0);
    bhg::PrefixOwner w;
    w.rho = o->rho;
    w.refused_run = o->refused_run;
    w.roomy_run = o->roomy_run;
    w.clean_run = o->clean_run;
    const int ask = w.next(rule, clear, a.r_hor, x0, n_spheres, last ? last->mode : BHG_PREFIX_NONE, last ? last->used : BHG_PREFIX_NONE,
                           last ? last->rho : 0.0, promote);
    o->rho = w.rho;
    o->clean_run = w.clean_run;
    o->refused_run = w.refused_run;
    o->roomy_run = w.roomy_run;
    return bhg::prefix_owner_fit_budget(ask, w.rho, a.r_hor, x0, a.max_steps);
}

// THE list of what a ray's initial step depends on beside the ray itself (initial_record, geodesic_kernels.hip): the
// controller's tolerances and limits and the metric.  The integrator is in it because only DP5(4) has such a step: a
// recording RK4 call leaves the array as it was.  Compared bit for bit (a -0.0 or another NaN counts as a change: safe).
int bhg_start_steps_match(const bhg_params *a, const bhg_params *b)
{
    if (!a || !b) return 0;
    auto same = [](double x, double y) { return std::memcmp(&x, &y, sizeof(double)) == 0; };
    return same(a->rtol, b->rtol) && same(a->atol, b->atol) && same(a->lambda_end, b->lambda_end) &&
           same(a->max_step, b->max_step) && same(a->r_s, b->r_s) && same(a->spin, b->spin) &&
           (a->time_like != 0) == (b->time_like != 0) && a->rhs_form == b->rhs_form && a->method == b->method;
}

// what the crossings trace covers, checked before the context (a refusal names its figure with or without a device)
static int crossings_check(const bhg_params *p, int32_t max_crossings)
{
    BHG_TRY(validate(p));
    if (p->method != BHG_METHOD_DP54) return fail(BHG_E_INVALID, "the crossings trace is DP5(4) only: method must be BHG_METHOD_DP54");
    if (p->time_like) return fail(BHG_E_INVALID, "the crossings trace covers null rays only: time_like must be 0");
    if (!(p->disk_r_out > 0.0)) return fail(BHG_E_INVALID, "the crossings trace needs a disk: disk_r_out must be > 0");
    if (max_crossings < 1 || max_crossings > BHG_MAX_CROSSINGS)
        return fail(BHG_E_INVALID, "max_crossings must be in [1, BHG_MAX_CROSSINGS]");
    return BHG_OK;
}

int bhg_trace_crossings_device(bhg_context *c, const bhg_params *p, const double *x0_shared, const double *d_x0,
                               const double *d_k0, size_t n, int32_t max_crossings, double *d_end, uint8_t *d_flags,
                               uint32_t *d_n_steps, uint32_t *d_n_accepted, double *d_cross, uint8_t *d_n_cross, void *stream)
{
    BHG_TRY(crossings_check(p, max_crossings));
    if (n && (!d_end || !d_cross || !d_n_cross)) return fail(BHG_E_INVALID, "end / cross / n_cross is NULL");
    return trace_device_impl(c, p, {.kind = TraceKind::CROSSINGS, .x0_shared = x0_shared, .d_x0 = d_x0, .d_k0 = d_k0, .n = n,
                                    .d_end = d_end, .d_flags = d_flags, .d_n_steps = d_n_steps, .d_n_accepted = d_n_accepted,
                                    .stream = stream, .cross = d_cross, .n_cross = d_n_cross, .max_cross = max_crossings, .stride = n});
}

// the host-buffer call, plain: upload, one device call, download (the crossings trace is not a streaming path)
int bhg_trace_crossings(bhg_context *c, const bhg_params *p, const double *x0, int x0_is_shared, const double *k0, size_t n,
                        int32_t max_crossings, double *end, uint8_t *flags, uint32_t *n_steps, uint32_t *n_accepted,
                        double *cross, uint8_t *n_cross)
{
    BHG_TRY(crossings_check(p, max_crossings));
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (n == 0) return BHG_OK;
    if (!x0 || !k0 || !end || !cross || !n_cross) return fail(BHG_E_INVALID, "x0 / k0 / end / cross / n_cross is NULL");
    if (n > 0xFFFFFFFFull) return fail(BHG_E_INVALID, "n must be < 2^32 per call");
    ENTER_DEVICE(c->device);
    const size_t b3 = n * 3 * sizeof(double), b6 = 2 * b3, bu = n * sizeof(uint32_t);
    Staged st(c, true);
    const size_t k = st.in(k0, b3), x = st.in(x0_is_shared ? nullptr : x0, b3), e = st.out(end, b6),
                 cr = st.inout(cross, (size_t)max_crossings * b6), nc = st.out(n_cross, n), fl = st.out(flags, n),
                 ns = st.out(n_steps, bu), na = st.out(n_accepted, bu);
    return st.run([&] {
        return bhg_trace_crossings_device(c, p, x0_is_shared ? x0 : nullptr, st.at<double>(x), st.at<double>(k), n, max_crossings,
                                          st.at<double>(e), st.at<uint8_t>(fl), st.at<uint32_t>(ns), st.at<uint32_t>(na),
                                          st.at<double>(cr), st.at<uint8_t>(nc), c->stream);
    });
}

// what the travel-time trace covers, checked before the context like the crossings trace's
static int travel_time_check(const bhg_params *p, int32_t max_crossings, const double *t_end)
{
    BHG_TRY(validate(p));
    if (p->method != BHG_METHOD_DP54) return fail(BHG_E_INVALID, "the travel-time trace is DP5(4) only: method must be BHG_METHOD_DP54");
    if (p->time_like) return fail(BHG_E_INVALID, "the travel-time trace covers null rays only: time_like must be 0");
    if (max_crossings < 0 || max_crossings > BHG_MAX_CROSSINGS)
        return fail(BHG_E_INVALID, "max_crossings must be in [0, BHG_MAX_CROSSINGS]");
    if (max_crossings > 0 && !(p->disk_r_out > 0.0))
        return fail(BHG_E_INVALID, "crossing times need a disk: disk_r_out must be > 0 when max_crossings > 0");
    if (!t_end) return fail(BHG_E_INVALID, "t_end is NULL");
    return BHG_OK;
}

int bhg_travel_time_device(bhg_context *c, const bhg_params *p, const double *x0_shared, const double *d_x0,
                           const double *d_k0, size_t n, int32_t max_crossings, double *d_end, uint8_t *d_flags,
                           uint32_t *d_n_steps, uint32_t *d_n_accepted, double *d_cross, uint8_t *d_n_cross, double *d_t_end,
                           double *d_t_cross, void *stream)
{
    BHG_TRY(travel_time_check(p, max_crossings, d_t_end));
    if (n && !d_end) return fail(BHG_E_INVALID, "end is NULL");
    if (n && max_crossings > 0 && (!d_cross || !d_n_cross || !d_t_cross))
        return fail(BHG_E_INVALID, "cross / n_cross / t_cross is NULL with max_crossings > 0");
    // (without records the kernel writes neither cross nor t_cross; n_cross is still counted when it is given and a disk is set)
    return trace_device_impl(c, p, {.kind = TraceKind::TRAVEL_TIME, .x0_shared = x0_shared, .d_x0 = d_x0, .d_k0 = d_k0, .n = n,
                                    .d_end = d_end, .d_flags = d_flags, .d_n_steps = d_n_steps, .d_n_accepted = d_n_accepted,
                                    .stream = stream, .cross = max_crossings > 0 ? d_cross : nullptr, .n_cross = d_n_cross,
                                    .max_cross = max_crossings, .stride = n, .t_end = d_t_end,
                                    .t_cross = max_crossings > 0 ? d_t_cross : nullptr});
}

// the host-buffer call, as bhg_trace_crossings: upload, one device call, download (cross, n_cross and t_cross may be NULL with
// max_crossings = 0)
int bhg_travel_time(bhg_context *c, const bhg_params *p, const double *x0, int x0_is_shared, const double *k0, size_t n,
                    int32_t max_crossings, double *end, uint8_t *flags, uint32_t *n_steps, uint32_t *n_accepted, double *cross,
                    uint8_t *n_cross, double *t_end, double *t_cross)
{
    BHG_TRY(travel_time_check(p, max_crossings, t_end));
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (n == 0) return BHG_OK;
    if (!x0 || !k0 || !end) return fail(BHG_E_INVALID, "x0 / k0 / end is NULL");
    if (max_crossings > 0 && (!cross || !n_cross || !t_cross))
        return fail(BHG_E_INVALID, "cross / n_cross / t_cross is NULL with max_crossings > 0");
    if (n > 0xFFFFFFFFull) return fail(BHG_E_INVALID, "n must be < 2^32 per call");
    ENTER_DEVICE(c->device);
    const size_t b3 = n * 3 * sizeof(double), b6 = 2 * b3, bu = n * sizeof(uint32_t), bt = n * sizeof(double);
    const bool records = max_crossings > 0;      // (without them cross and t_cross stay on the host, and n_cross is optional)
    Staged st(c, true);
    const size_t k = st.in(k0, b3), x = st.in(x0_is_shared ? nullptr : x0, b3), e = st.out(end, b6), te = st.out(t_end, bt),
                 cr = st.inout(records ? cross : nullptr, (size_t)max_crossings * b6),
                 tc = st.inout(records ? t_cross : nullptr, (size_t)max_crossings * bt),
                 nc = n_cross ? st.out(n_cross, n) : Staged::NONE, fl = st.out(flags, n), ns = st.out(n_steps, bu),
                 na = st.out(n_accepted, bu);
    return st.run([&] {
        return bhg_travel_time_device(c, p, x0_is_shared ? x0 : nullptr, st.at<double>(x), st.at<double>(k), n, max_crossings,
                                      st.at<double>(e), st.at<uint8_t>(fl), st.at<uint32_t>(ns), st.at<uint32_t>(na), st.at<double>(cr),
                                      st.at<uint8_t>(nc), st.at<double>(te), st.at<double>(tc), c->stream);
    });
}

// --- triangle meshes: the trace; bhgeo_mesh.hip has the mesh itself -------------------------------------

int bhg_trace_mesh_device(bhg_context *c, const bhg_params *p, const bhg_mesh *mesh, double max_chord, const double *x0_shared,
                          const double *d_x0, const double *d_k0, size_t n, double *d_end, uint8_t *d_flags, uint32_t *d_n_steps,
                          uint32_t *d_n_accepted, int32_t *d_tri_id, double *d_bary, void *stream)
{
    BHG_TRY(bhg::mesh_trace_check(p, mesh, max_chord, d_tri_id, d_bary));
    BHG_TRY(bhg::mesh_on_device_of(c, mesh));
    if (n && !d_end) return fail(BHG_E_INVALID, "end is NULL");
    return trace_device_impl(c, p, {.kind = TraceKind::MESH, .x0_shared = x0_shared, .d_x0 = d_x0, .d_k0 = d_k0, .n = n, .d_end = d_end,
                                    .d_flags = d_flags, .d_n_steps = d_n_steps, .d_n_accepted = d_n_accepted, .stream = stream,
                                    .stride = n, .mesh = mesh, .max_chord = max_chord, .tri_id = d_tri_id, .bary = d_bary});
}

// the host-buffer call, as bhg_trace_crossings: upload, one device call, download.  bary is read first (a ray that hits nothing
// leaves its slot as it was).  Blocking.
int bhg_trace_mesh(bhg_context *c, const bhg_params *p, const bhg_mesh *mesh, double max_chord, const double *x0, int x0_is_shared,
                   const double *k0, size_t n, double *end, uint8_t *flags, uint32_t *n_steps, uint32_t *n_accepted, int32_t *tri_id,
                   double *bary)
{
    BHG_TRY(bhg::mesh_trace_check(p, mesh, max_chord, tri_id, bary));
    BHG_TRY(bhg::mesh_on_device_of(c, mesh));
    if (n == 0) return BHG_OK;
    if (!x0 || !k0 || !end) return fail(BHG_E_INVALID, "x0 / k0 / end is NULL");
    if (n > 0xFFFFFFFFull) return fail(BHG_E_INVALID, "n must be < 2^32 per call");
    ENTER_DEVICE(c->device);
    const size_t b3 = n * 3 * sizeof(double), b6 = 2 * b3, bu = n * sizeof(uint32_t);
    Staged st(c, true);
    const size_t k = st.in(k0, b3), x = st.in(x0_is_shared ? nullptr : x0, b3), e = st.out(end, b6), tr = st.out(tri_id, bu),
                 ba = st.inout(bary, n * 2 * sizeof(double)), fl = st.out(flags, n), ns = st.out(n_steps, bu),
                 na = st.out(n_accepted, bu);
    return st.run([&] {
        return bhg_trace_mesh_device(c, p, mesh, max_chord, x0_is_shared ? x0 : nullptr, st.at<double>(x), st.at<double>(k), n,
                                     st.at<double>(e), st.at<uint8_t>(fl), st.at<uint32_t>(ns), st.at<uint32_t>(na),
                                     st.at<int32_t>(tr), st.at<double>(ba), c->stream);
    });
}

// ... and of the rigid placements of a mesh
int bhg_trace_mesh_instances_device(bhg_context *c, const bhg_params *p, const bhg_mesh_instances *inst, double max_chord,
                                    const double *x0_shared, const double *d_x0, const double *d_k0, size_t n, double *d_end,
                                    uint8_t *d_flags, uint32_t *d_n_steps, uint32_t *d_n_accepted, int32_t *d_tri_id,
                                    int32_t *d_inst_id, double *d_bary, void *stream)
{
    BHG_TRY(bhg::instances_trace_check(p, inst, max_chord, d_tri_id, d_inst_id, d_bary));
    BHG_TRY(bhg::instances_usable(c, inst));
    if (n && !d_end) return fail(BHG_E_INVALID, "end is NULL");
    return trace_device_impl(c, p, {.kind = TraceKind::MESH, .x0_shared = x0_shared, .d_x0 = d_x0, .d_k0 = d_k0, .n = n, .d_end = d_end,
                                    .d_flags = d_flags, .d_n_steps = d_n_steps, .d_n_accepted = d_n_accepted, .stream = stream,
                                    .stride = n, .mesh = inst->mesh, .max_chord = max_chord, .tri_id = d_tri_id, .bary = d_bary,
                                    .instances = inst, .inst_id = d_inst_id});
}

int bhg_trace_mesh_instances(bhg_context *c, const bhg_params *p, const bhg_mesh_instances *inst, double max_chord, const double *x0,
                             int x0_is_shared, const double *k0, size_t n, double *end, uint8_t *flags, uint32_t *n_steps,
                             uint32_t *n_accepted, int32_t *tri_id, int32_t *inst_id, double *bary)
{
    BHG_TRY(bhg::instances_trace_check(p, inst, max_chord, tri_id, inst_id, bary));
    BHG_TRY(bhg::instances_usable(c, inst));
    if (n == 0) return BHG_OK;
    if (!x0 || !k0 || !end) return fail(BHG_E_INVALID, "x0 / k0 / end is NULL");
    if (n > 0xFFFFFFFFull) return fail(BHG_E_INVALID, "n must be < 2^32 per call");
    ENTER_DEVICE(c->device);
    const size_t b3 = n * 3 * sizeof(double), b6 = 2 * b3, bu = n * sizeof(uint32_t);
    Staged st(c, true);
    const size_t k = st.in(k0, b3), x = st.in(x0_is_shared ? nullptr : x0, b3), e = st.out(end, b6), tr = st.out(tri_id, bu),
                 ii = st.out(inst_id, bu), ba = st.inout(bary, n * 2 * sizeof(double)), fl = st.out(flags, n),
                 ns = st.out(n_steps, bu), na = st.out(n_accepted, bu);
    return st.run([&] {
        return bhg_trace_mesh_instances_device(c, p, inst, max_chord, x0_is_shared ? x0 : nullptr, st.at<double>(x), st.at<double>(k),
                                               n, st.at<double>(e), st.at<uint8_t>(fl), st.at<uint32_t>(ns), st.at<uint32_t>(na),
                                               st.at<int32_t>(tr), st.at<int32_t>(ii), st.at<double>(ba), c->stream);
    });
}

int bhg_trace(bhg_context *c, const bhg_params *p, const double *x0, int x0_is_shared, const double *k0,
              size_t n, double *end, uint8_t *flags, uint32_t *n_steps, uint32_t *n_accepted)
{
    return bhg_trace_objects(c, p, nullptr, 0, x0, x0_is_shared, k0, n, end, flags, n_steps, n_accepted, nullptr);
}

}  // extern "C"

struct bhg_rays {
    bhg_context *ctx = nullptr;
    double *d_k0 = nullptr;  // [n][3], ray s * n_pixels + p = sample s of pixel p
    size_t n = 0;
    double origin[3] = {0, 0, 0};
};

namespace {

// what a pipelined call reads and writes on the host side
struct PipeIO {
    const double *h_k0 = nullptr, *h_x0 = nullptr;  // caller's rays (h_x0: per-ray origins) ...
    const double *d_k0 = nullptr;                   // ... or rays already resident on the device (no upload)
    const double *x0_shared = nullptr;              // host [3] when the origin is shared
    double *end = nullptr, *loc = nullptr, *dir = nullptr;  // end [n][6] and / or its halves [n][3]
    uint8_t *flags = nullptr;
    uint32_t *steps = nullptr, *acc = nullptr;
    int8_t *obj = nullptr;
};

// The host-buffer calls as a pipeline over chunks of rays:
//   host   : caller's k0 (x0) chunk -> pinned ring          (worker threads; skipped for pinned caller memory)
//   s_in   : H2D                                            (copy engine; nothing to do for resident rays)
//   stream : trace (one launch per chunk), end -> loc / dir (compute)
//   s_out  : D2H of the arrays the caller asked for         (the other copy engine)
//   host   : pinned ring -> caller's arrays                 (worker threads; skipped for pinned caller memory)
// Chunk c+1 is staged and uploaded while chunk c is traced and chunk c-1 comes back.  Results do not depend on the
// chunking: every ray is its own ODE.
int pipeline_impl(bhg_context *c, const bhg_params *p, const double *spheres, int32_t n_spheres, const PipeIO &io, size_t n)
{
    ENTER_DEVICE(c->device);
    if (!c->s_in) {
        HIP_TRY(hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) {
            HIP_TRY(hipEventCreateWithFlags(&c->ev_in[i], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&c->ev_k[i], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&c->ev_out[i], hipEventDisableTiming));
        }
    }
    // Whatever way this call ends, nothing of it may still be running when it returns: copies and kernels of earlier
    // chunks DMA into the caller's page-locked arrays and into the pinned ring, and the next call's ensure() may free
    // buffers they use.  (The success path has waited already; the guard then costs three no-op synchronisations.)
    struct StreamsQuiet {
        bhg_context *c;
        ~StreamsQuiet()
        {
            if (c->s_in) (void)hipStreamSynchronize(c->s_in);
            if (c->stream) (void)hipStreamSynchronize(c->stream);
            if (c->s_out) (void)hipStreamSynchronize(c->s_out);
        }
    } quiet{c};
    const bool upload = io.d_k0 == nullptr;
    const bool per_ray_x0 = io.h_x0 != nullptr;
    const bool dir_only = io.dir && !io.end && !io.loc;   // the trace writes the directions itself: no records, no split pass
    const bool split = (io.loc || io.dir) && !dir_only;
    // device arrays for the whole call (chunks are sub-ranges of each)
    const size_t in_bytes = upload ? n * 3 * sizeof(double) * (per_ray_x0 ? 2 : 1) : 0;
    const size_t off_flags = dir_only ? 0 : n * 6 * sizeof(double);   // (no record array in a direction-only call)
    const size_t off_steps = off_flags + ((n + 7) & ~size_t(7));
    const size_t off_acc = off_steps + n * sizeof(uint32_t);
    const size_t off_obj = off_acc + n * sizeof(uint32_t);
    const size_t off_loc = (off_obj + n + 7) & ~size_t(7);
    const size_t off_dir = off_loc + (split ? n * 3 * sizeof(double) : 0);
    const size_t out_bytes = off_dir + ((split || dir_only) ? n * 3 * sizeof(double) : 0);
    int rc = BHG_OK;
    if (upload) {
        rc = ensure(&c->d_in, &c->d_in_bytes, in_bytes);
        if (rc != BHG_OK) return rc;
    }
    rc = ensure(&c->d_out, &c->d_out_bytes, out_bytes);
    if (rc != BHG_OK) return rc;
    double *d_k0u = (double *)c->d_in;
    const double *d_k0 = upload ? d_k0u : io.d_k0;
    double *d_x0 = per_ray_x0 ? d_k0u + n * 3 : nullptr;
    char *o = (char *)c->d_out;
    double *d_end = (double *)o, *d_loc = (double *)(o + off_loc), *d_dir = (double *)(o + off_dir);
    uint8_t *d_flags = (uint8_t *)(o + off_flags);
    uint32_t *d_steps = (uint32_t *)(o + off_steps), *d_acc = (uint32_t *)(o + off_acc);
    int8_t *d_obj = io.obj ? (int8_t *)(o + off_obj) : nullptr;

    const size_t chunk = size_t(1) << 20;  // rays per chunk: 24 MB up, 57 MB back
    const size_t n_chunks = (n + chunk - 1) / chunk;
    const size_t cmax = std::min(chunk, n);
    const bool pin_k0 = !upload || is_pinned(io.h_k0), pin_x0 = !per_ray_x0 || is_pinned(io.h_x0);
    struct OutArr {
        void *host;
        const char *dev;
        size_t elem;
        bool pinned;
        size_t ring_off;
    } outs[7] = {{io.end, (const char *)d_end, 48, false, 0},   {io.loc, (const char *)d_loc, 24, false, 0},
                 {io.dir, (const char *)d_dir, 24, false, 0},   {io.flags, (const char *)d_flags, 1, false, 0},
                 {io.steps, (const char *)d_steps, 4, false, 0}, {io.acc, (const char *)d_acc, 4, false, 0},
                 {io.obj, (const char *)d_obj, 1, false, 0}};
    size_t so_slot = 0;
    bool stage_out = false;
    for (auto &a : outs) {
        if (!a.host) continue;
        a.pinned = is_pinned(a.host);
        a.ring_off = so_slot;
        so_slot += (cmax * a.elem + 63) & ~size_t(63);
        stage_out = stage_out || !a.pinned;
    }
    const size_t si_x0 = cmax * 24, si_slot = cmax * 48;
    if (!pin_k0 || !pin_x0) {
        rc = ensure_pinned(&c->pin_in, &c->pin_in_bytes, 2 * si_slot);
        if (rc != BHG_OK) return rc;
    }
    if (stage_out) {
        rc = ensure_pinned(&c->pin_out, &c->pin_out_bytes, 2 * so_slot);
        if (rc != BHG_OK) return rc;
    }

    auto copy_out = [&](size_t ch) -> int {  // host side of chunk ch's way back
        const int slot = (int)(ch & 1);
        const size_t off = ch * chunk, m = std::min(chunk, n - off);
        HIP_TRY(hipEventSynchronize(c->ev_out[slot]));
        const char *ps = (const char *)c->pin_out + (size_t)slot * so_slot;
        for (auto &a : outs)
            if (a.host && !a.pinned) c->pool.copy((char *)a.host + off * a.elem, ps + a.ring_off, m * a.elem);
        return BHG_OK;
    };

    for (size_t ch = 0; ch < n_chunks; ch++) {
        const int slot = (int)(ch & 1);
        const size_t off = ch * chunk, m = std::min(chunk, n - off);
        if (upload) {
            char *pi = (char *)c->pin_in + (size_t)slot * si_slot;
            // the slot's previous upload (chunk ch - 2) must have left the staging memory
            if (ch >= 2 && (!pin_k0 || !pin_x0)) HIP_TRY(hipEventSynchronize(c->ev_in[slot]));
            const void *src_k0 = io.h_k0 + off * 3, *src_x0 = per_ray_x0 ? io.h_x0 + off * 3 : nullptr;
            if (!pin_k0) {
                c->pool.copy(pi, src_k0, m * 24);
                src_k0 = pi;
            }
            if (per_ray_x0 && !pin_x0) {
                c->pool.copy(pi + si_x0, src_x0, m * 24);
                src_x0 = pi + si_x0;
            }
            HIP_TRY(hipMemcpyAsync(d_k0u + off * 3, src_k0, m * 24, hipMemcpyHostToDevice, c->s_in));
            if (per_ray_x0) HIP_TRY(hipMemcpyAsync(d_x0 + off * 3, src_x0, m * 24, hipMemcpyHostToDevice, c->s_in));
            HIP_TRY(hipEventRecord(c->ev_in[slot], c->s_in));
            HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_in[slot], 0));
        }
        rc = trace_device_impl(c, p, {.spheres = spheres, .n_spheres = n_spheres, .x0_shared = io.x0_shared,
                                      .d_x0 = per_ray_x0 ? d_x0 + off * 3 : nullptr, .d_k0 = d_k0 + off * 3, .n = m,
                                      .d_end = dir_only ? nullptr : d_end + off * 6, .d_end_dir = dir_only ? d_dir + off * 3 : nullptr,
                                      .d_flags = d_flags + off, .d_n_steps = d_steps + off, .d_n_accepted = d_acc + off,
                                      .d_object_id = d_obj ? d_obj + off : nullptr, .stream = c->stream});
        if (rc != BHG_OK) return rc;
        if (split)
            HIP_TRY(bhg::launch_split_end(d_end + off * 6, m, io.loc ? d_loc + off * 3 : nullptr, io.dir ? d_dir + off * 3 : nullptr,
                                          c->stream));
        HIP_TRY(hipEventRecord(c->ev_k[slot], c->stream));
        HIP_TRY(hipStreamWaitEvent(c->s_out, c->ev_k[slot], 0));
        char *po = (char *)c->pin_out + (size_t)slot * so_slot;
        for (auto &a : outs)
            if (a.host)
                HIP_TRY(hipMemcpyAsync(a.pinned ? (void *)((char *)a.host + off * a.elem) : (void *)(po + a.ring_off),
                                       a.dev + off * a.elem, m * a.elem, hipMemcpyDeviceToHost, c->s_out));
        HIP_TRY(hipEventRecord(c->ev_out[slot], c->s_out));
        // while the GPU works on this chunk: the previous chunk's results go from the ring to the caller's arrays
        if (ch >= 1) {
            rc = copy_out(ch - 1);
            if (rc != BHG_OK) return rc;
        }
    }
    rc = copy_out(n_chunks - 1);
    if (rc != BHG_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->s_out));
    return BHG_OK;
}

}  // namespace

extern "C" {

int bhg_trace_objects(bhg_context *c, const bhg_params *p, const double *spheres, int32_t n_spheres, const double *x0,
                      int x0_is_shared, const double *k0, size_t n, double *end, uint8_t *flags, uint32_t *n_steps,
                      uint32_t *n_accepted, int8_t *object_id)
{
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    BHG_TRY(validate(p));
    BHG_TRY(validate_spheres(p, spheres, n_spheres));
    if (n == 0) return BHG_OK;
    if (!x0 || !k0 || !end) return fail(BHG_E_INVALID, "x0 / k0 / end is NULL");
    if (n > 0xFFFFFFFFull) return fail(BHG_E_INVALID, "n must be < 2^32 per call");
    PipeIO io;
    io.h_k0 = k0;
    io.h_x0 = x0_is_shared ? nullptr : x0;
    io.x0_shared = x0_is_shared ? x0 : nullptr;
    io.end = end;
    io.flags = flags;
    io.steps = n_steps;
    io.acc = n_accepted;
    io.obj = object_id;
    return pipeline_impl(c, p, spheres, n_spheres, io, n);
}

/* ---- rays resident on the device ------------------------------------------------------- */
int bhg_rays_create(bhg_context *c, const bhg_camera *cam, const double *jitter, int jitter_is_compact, const int64_t *pixels,
                    size_t n_pixels, bhg_rays **out)
{
    if (!out) return fail(BHG_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!c || !cam) return fail(BHG_E_INVALID, "ctx / camera is NULL");
    if (cam->width <= 0 || cam->height <= 0 || cam->samples <= 0) return fail(BHG_E_INVALID, "width, height, samples must be > 0");
    const size_t frame_px = (size_t)cam->width * (size_t)cam->height;
    if (!pixels) n_pixels = frame_px;
    if (n_pixels == 0) {
        // an empty pixel list -- a shard that was dealt no tile (more devices than tiles) -- is a ray set of 0 rays:
        // bhg_rays_count() = 0, bhg_rays_trace(..., 0, 0, ...) a no-op
        bhg_rays *r0 = new (std::nothrow) bhg_rays();
        if (!r0) return fail(BHG_E_NOMEM, "host allocation failed");
        r0->ctx = c;
        r0->n = 0;
        std::memcpy(r0->origin, cam->origin, sizeof(r0->origin));
        *out = r0;
        return BHG_OK;
    }
    if (jitter_is_compact && !jitter) return fail(BHG_E_INVALID, "compact jitter stream is NULL");
    const size_t n = n_pixels * (size_t)cam->samples;
    if (n > 0xFFFFFFFFull) return fail(BHG_E_INVALID, "more than 2^32 rays");
    ENTER_DEVICE(c->device);
    bhg_rays *r = new (std::nothrow) bhg_rays();
    if (!r) return fail(BHG_E_NOMEM, "host allocation failed");
    r->ctx = c;
    r->n = n;
    std::memcpy(r->origin, cam->origin, sizeof(r->origin));
    hipError_t e = hipMalloc((void **)&r->d_k0, n * 3 * sizeof(double));
    if (e != hipSuccess) {
        delete r;
        return fail_hip(e, "hipMalloc(rays)");
    }
    // the jitter stream and the pixel list are only needed to generate the rays: staged in the call's own buffers
    const size_t n_jit = jitter ? 2 * (size_t)cam->samples * (jitter_is_compact ? n_pixels : frame_px) : 0;
    const size_t tmp_bytes = n_jit * sizeof(double) + (pixels ? n_pixels * sizeof(int64_t) : 0);
    int rc = ensure(&c->d_in, &c->d_in_bytes, tmp_bytes + 64);
    if (rc != BHG_OK) {
        (void)hipFree(r->d_k0);
        delete r;
        return rc;
    }
    double *d_jit = (double *)c->d_in;
    int64_t *d_pix = (int64_t *)((char *)c->d_in + n_jit * sizeof(double));
    bhg::RaygenArgs a;
    std::memset(&a, 0, sizeof(a));
    hipError_t err = hipSuccess;
    if (jitter) err = hipMemcpyAsync(d_jit, jitter, n_jit * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (err == hipSuccess && pixels) err = hipMemcpyAsync(d_pix, pixels, n_pixels * sizeof(int64_t), hipMemcpyHostToDevice, c->stream);
    a.jitter = jitter ? d_jit : nullptr;
    a.compact = jitter_is_compact ? 1 : 0;
    a.pixels = pixels ? d_pix : nullptr;
    a.k0 = r->d_k0;
    a.n_pixels = n_pixels;
    a.width = cam->width;
    a.height = cam->height;
    a.samples = cam->samples;
    a.fov_x = cam->fov_x;
    a.fov_y = cam->fov_y;
    static const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    a.rotate = std::memcmp(cam->rot, eye, sizeof(eye)) != 0;
    std::memcpy(a.rot, cam->rot, sizeof(a.rot));
    if (err == hipSuccess) err = bhg::launch_raygen(a, c->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) {
        (void)hipFree(r->d_k0);
        delete r;
        return fail_hip(err, "ray generation");
    }
    *out = r;
    return BHG_OK;
}

size_t bhg_rays_count(const bhg_rays *r) { return r ? r->n : 0; }

void bhg_rays_destroy(bhg_rays *r)
{
    if (!r) return;
    if (r->d_k0) {
        DeviceGuard guard(r->ctx->device);
        (void)hipFree(r->d_k0);
    }
    delete r;
}

int bhg_rays_trace(bhg_rays *r, const bhg_params *p, const double *spheres, int32_t n_spheres, size_t first, size_t n,
                   double *end, double *end_loc, double *end_dir, uint8_t *flags, uint32_t *n_steps, uint32_t *n_accepted,
                   int8_t *object_id)
{
    if (!r) return fail(BHG_E_INVALID, "rays is NULL");
    BHG_TRY(validate(p));
    BHG_TRY(validate_spheres(p, spheres, n_spheres));
    if (first > r->n || n > r->n - first) return fail(BHG_E_INVALID, "ray range out of bounds");
    if (n == 0) return BHG_OK;
    if (!end && !end_loc && !end_dir && !flags) return fail(BHG_E_INVALID, "no result array given");
    PipeIO io;
    io.d_k0 = r->d_k0 + first * 3;
    io.x0_shared = r->origin;
    io.end = end;
    io.loc = end_loc;
    io.dir = end_dir;
    io.flags = flags;
    io.steps = n_steps;
    io.acc = n_accepted;
    io.obj = object_id;
    return pipeline_impl(r->ctx, p, spheres, n_spheres, io, n);
}

int bhg_host_alloc(bhg_context *c, size_t bytes, void **out)
{
    if (!out) return fail(BHG_E_INVALID, "out is NULL");
    *out = nullptr;
    if (bytes == 0) return BHG_OK;
    if (c) {   // with the owning context's device current; without a context: whatever device the caller is on
        ENTER_DEVICE(c->device);
        HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
        return BHG_OK;
    }
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return BHG_OK;
}

int bhg_host_free(bhg_context *c, void *p)
{
    (void)c;
    if (!p) return BHG_OK;
    HIP_TRY(hipHostFree(p));
    return BHG_OK;
}

}  // extern "C"

namespace {
int raygen_impl(bhg_context *c, int32_t width, int32_t height, int32_t samples, double fov_x, double fov_y,
                const double *rot9, const double *d_jitter, const int64_t *d_pixels, size_t n_pixels,
                double *d_k0, void *stream, const bhg::ObserverParams *obs)
{
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (width <= 0 || height <= 0 || samples <= 0) return fail(BHG_E_INVALID, "width, height, samples must be > 0");
    if (n_pixels == 0) return BHG_OK;
    if (!d_jitter || !d_k0) return fail(BHG_E_INVALID, "jitter / k0 is NULL");
    if (!d_pixels && n_pixels != (size_t)width * (size_t)height)
        return fail(BHG_E_INVALID, "n_pixels must be width*height when no pixel list is given");
    ENTER_DEVICE(c->device);
    bhg::RaygenArgs a;
    std::memset(&a, 0, sizeof(a));
    a.jitter = d_jitter;
    a.pixels = d_pixels;
    a.k0 = d_k0;
    a.n_pixels = n_pixels;
    a.width = width;
    a.height = height;
    a.samples = samples;
    a.fov_x = fov_x;
    a.fov_y = fov_y;
    a.rotate = 0;
    if (rot9) {
        static const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        a.rotate = std::memcmp(rot9, eye, sizeof(eye)) != 0;
        std::memcpy(a.rot, rot9, sizeof(a.rot));
    }
    if (obs) a.obs = *obs;
    HIP_TRY(bhg::launch_raygen(a, (hipStream_t)stream));
    return BHG_OK;
}

// The one shade call: every bhg_shade*_device is this with some arguments NULL (include/bhgeo.h).  Its checks run in one
// order, whichever entry point was taken, so that settings are refused with or without a device:
//   1. the scene: present; samples, sky_w, sky_h > 0; n_spheres in [0, BHG_MAX_SPHERES], n_lamps in [0, 4]; a disk with
//      r_out > r_in, stddev > 0 and a texture size > 0; sphere radii > 0
//   2. the object-texture table, when given, against n_spheres
//   2b. the object motion, when given, against n_spheres and the trace parameters (finite; moving spheres outside the horizon
//      and timelike on the whole sphere)
//   3. redshift, when rs->apply != 0: x0_shared, the settings, and the observer when given
//   3b. polarisation, when pol is given: x0_shared, the settings (against p, the scene's disk, the redshift's sense, the camera)
//   3c. the thermal disk, when th is given: the settings (against p, the scene's disk, the redshift's and polarisation's
//      sense), x0_shared and the camera, and the observer when given
//   4. the context
//   5. n_pixels == 0 is BHG_OK: an EMPTY shard -- a rank without pixels: fewer tiles than ranks -- has no rays and no
//      arrays, so no device array is looked at
//   6. the device arrays: an output, end or end_dir, flags, the sky; end for a disk or spheres; object_id for spheres;
//      k0 for redshift; qu and k0 for polarisation; k0 for the thermal disk
// layered: the call is the layered shade of a crossings trace (bhg_shade_disk_layers_device): checked after the scene (step 1b: a
// disk, no spheres, max_crossings, opacity), its arrays with the others in step 6
struct ShadeCall {
    const double *end = nullptr, *end_dir = nullptr;   // [n][6], or -- end null -- [n][3]
    const uint8_t *flags = nullptr;
    const int8_t *object_id = nullptr;
    size_t n_pixels = 0;
    int32_t samples = 0;
    const bhg_scene *sc = nullptr;       // the settings: all but the scene may be NULL
    const bhg_params *p = nullptr;
    const bhg_redshift *rs = nullptr;
    const bhg_observer *obs = nullptr;
    const bhg_object_textures *ot = nullptr;
    const double *x0_shared = nullptr, *k0 = nullptr;
    double *rgba = nullptr;
    float *rgba_f32 = nullptr;
    const int64_t *scatter = nullptr;
    const bhg_polarisation *pol = nullptr;
    double *qu = nullptr;
    const bhg_disk_thermal *th = nullptr;
    const bhg_object_motion *mo = nullptr;
    void *stream = nullptr;
    bool layered = false;
    const double *cross = nullptr;
    const uint8_t *n_cross = nullptr;
    const bhg_disk_layers *layers = nullptr;
    // the retarded shade (bhg_shade_disk_layers_retarded_device): nullptr / 0 = the plain layered shade's kernels
    const double *t_cross = nullptr;
    double phase_rate = 0.0;
};

// step 1 of shade()'s checks, and the mesh shade's (which goes with no object spheres and says so in its own words): the scene
// is there; samples and the sky's size; spheres and lamps; the disk
int scene_check(const bhg_scene *sc, int32_t samples, bool mesh)
{
    if (!sc) return fail(BHG_E_INVALID, "scene is NULL");
    if (samples <= 0 || sc->sky_w <= 0 || sc->sky_h <= 0) return fail(BHG_E_INVALID, "samples, sky_w, sky_h must be > 0");
    if (mesh) {
        if (sc->n_spheres != 0) return fail(BHG_E_INVALID, "the mesh shade does not go with object spheres: n_spheres must be 0");
        if (sc->n_lamps < 0 || sc->n_lamps > 4) return fail(BHG_E_INVALID, "n_lamps must be in [0, 4]");
    } else if (sc->n_spheres < 0 || sc->n_spheres > BHG_MAX_SPHERES || sc->n_lamps < 0 || sc->n_lamps > 4) {
        return fail(BHG_E_INVALID, "n_spheres must be in [0, BHG_MAX_SPHERES], n_lamps in [0, 4]");
    }
    if (sc->disk_r_out > 0.0) {
        if (!(sc->disk_r_out > sc->disk_r_in) || !(sc->disk_stddev > 0.0))
            return fail(BHG_E_INVALID, "disk needs r_out > r_in and stddev > 0");
        if (sc->d_disk_tex && (sc->disk_w <= 0 || sc->disk_h <= 0)) return fail(BHG_E_INVALID, "disk texture size must be > 0");
    }
    return BHG_OK;
}

// the scene's sky, disk and lamps into the kernels' arguments (the spheres are shade()'s own)
void fill_scene_args(bhg::ShadeArgs &a, const bhg_scene *sc)
{
    a.sky = sc->d_sky;
    a.sky_w = sc->sky_w;
    a.sky_h = sc->sky_h;
    a.disk_tex = sc->d_disk_tex;
    a.disk_w = sc->disk_w;
    a.disk_h = sc->disk_h;
    a.disk_r_in = sc->disk_r_in;
    a.disk_r_out = sc->disk_r_out;
    a.disk_phase = sc->disk_phase;
    a.disk_mean = sc->disk_mean;
    a.disk_stddev = sc->disk_stddev;
    a.disk_intensity = sc->disk_intensity;
    a.n_lamps = sc->n_lamps;
    std::memcpy(a.lamps, sc->lamps, sizeof(a.lamps));
}

int shade(bhg_context *c, const ShadeCall &s)
{
    const bhg_scene *const sc = s.sc;
    BHG_TRY(scene_check(sc, s.samples, false));
    const bool has_disk = sc->disk_r_out > 0.0;
    for (int j = 0; j < sc->n_spheres; j++)
        if (!(sc->spheres[j][3] > 0.0)) return fail(BHG_E_INVALID, "sphere radii must be > 0");
    if (s.layered) {
        if (!s.layers) return fail(BHG_E_INVALID, "disk layers: the settings are NULL");
        if (!has_disk) return fail(BHG_E_INVALID, "disk layers need a disk in the scene: disk_r_out must be > 0");
        if (sc->n_spheres > 0) return fail(BHG_E_INVALID, "disk layers do not go with object spheres: n_spheres must be 0");
        if (s.layers->max_crossings < 1 || s.layers->max_crossings > BHG_MAX_CROSSINGS)
            return fail(BHG_E_INVALID, "disk layers: max_crossings must be in [1, BHG_MAX_CROSSINGS]");
        if (!(s.layers->opacity > 0.0) || !(s.layers->opacity <= 1.0))
            return fail(BHG_E_INVALID, "disk layers: opacity must be in (0, 1]");
    }
    bhg::ObjectTextureParams tp;
    if (s.ot) {
        BHG_TRY(bhg::object_texture_params(s.ot, sc->n_spheres, &tp));
    }
    bhg::MotionParams mp;
    if (s.mo) {
        BHG_TRY(bhg::motion_params(s.p, s.mo, &sc->spheres[0][0], sc->n_spheres, &mp));
    }
    const bool on = s.rs && s.rs->apply != 0;
    bhg::RedshiftParams rp;
    bhg::ObserverParams op;
    if (on) {
        if (!s.x0_shared) return fail(BHG_E_INVALID, "x0_shared is NULL");
        BHG_TRY(bhg::redshift_params(s.p, s.rs, has_disk && (s.rs->apply & BHG_REDSHIFT_DISK) ? sc->disk_r_in : -1.0, s.x0_shared, &rp));
        if (s.obs) {
            BHG_TRY(bhg::observer_params(s.p, s.obs, s.x0_shared, &op));
        }
    }
    bhg::PolarisationParams pp;
    if (s.pol) {
        if (!s.x0_shared) return fail(BHG_E_INVALID, "polarisation needs the shared camera origin x0_shared");
        BHG_TRY(bhg::polarisation_params(s.p, s.pol, on ? s.rs : nullptr, s.obs, has_disk ? sc->disk_r_in : -1.0, s.x0_shared, &pp));
        if (s.obs) {
            bhg::ObserverParams chk;
            BHG_TRY(bhg::observer_params(s.p, s.obs, s.x0_shared, &chk));
        }
    }
    bhg::ThermalParams tp_th;
    bhg::RedshiftParams rp_th;
    bhg::ObserverParams op_th;
    if (s.th) {
        BHG_TRY(bhg::thermal_params(s.p, s.th, on ? s.rs : nullptr, s.pol, has_disk ? sc->disk_r_in : -1.0, s.x0_shared, &tp_th, &rp_th));
        if (!s.x0_shared) return fail(BHG_E_INVALID, "the thermal disk needs the shared camera origin x0_shared");
        if (s.obs) {
            BHG_TRY(bhg::observer_params(s.p, s.obs, s.x0_shared, &op_th));
        }
    }
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (s.n_pixels == 0) return BHG_OK;
    if ((!s.rgba && !s.rgba_f32) || (!s.end && !s.end_dir) || !s.flags || !sc->d_sky)
        return fail(BHG_E_INVALID, "NULL device pointer");
    if (s.layered && (!s.cross || !s.n_cross)) return fail(BHG_E_INVALID, "disk layers: d_cross / d_n_cross is NULL");
    // (the layered shade takes a disk ray's position from the crossing records: directions alone do for the rest)
    if (!s.end && ((has_disk && !s.layered) || sc->n_spheres > 0))
        return fail(BHG_E_INVALID, "d_end is NULL: a direction-only frame cannot have a disk or object spheres");
    if (sc->n_spheres > 0 && !s.object_id) return fail(BHG_E_INVALID, "object_id is NULL but the scene has spheres");
    if (on && !s.k0) return fail(BHG_E_INVALID, "redshift needs the camera directions d_k0");
    if (s.pol && (!s.qu || !s.k0)) return fail(BHG_E_INVALID, "polarisation needs d_qu and the camera directions d_k0");
    if (s.th && !s.k0) return fail(BHG_E_INVALID, "the thermal disk needs the camera directions d_k0");
    ENTER_DEVICE(c->device);
    bhg::ShadeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.end = s.end;
    a.dir = s.end ? nullptr : s.end_dir;
    if (on) {
        a.rs = rp;
        a.k0 = s.k0;
        if (s.obs) a.obs = op;
    }
    a.flags = s.flags;
    a.rgba = s.rgba;
    a.rgba_f32 = s.rgba_f32;
    a.scatter = s.scatter;
    a.n_pixels = s.n_pixels;
    a.samples = s.samples;
    fill_scene_args(a, sc);
    a.object_id = sc->n_spheres > 0 ? s.object_id : nullptr;
    a.n_spheres = sc->n_spheres;
    std::memcpy(a.spheres, sc->spheres, sizeof(a.spheres));
    std::memcpy(a.sphere_rgb, sc->sphere_rgb, sizeof(a.sphere_rgb));
    if (s.ot) a.ot = tp;
    if (s.pol) {
        a.pol = pp;
        a.pol.qu = s.qu;
        a.k0 = s.k0;
    }
    if (s.th) {
        // the redshift instance, always: the disk's g from rs (metric, camera, sense), objects and sky as the caller's apply
        a.th = tp_th;
        if (!on) a.rs = rp_th;
        a.k0 = s.k0;
        if (s.obs) a.obs = op_th;
    }
    if (s.mo) a.mo = mp;     // (launch_shade takes the motion instance only when rs.apply weighs objects)
    if (s.layered) {
        a.cross = s.cross;
        a.n_cross = s.n_cross;
        a.max_cross = s.layers->max_crossings;
        a.transmit = 1.0 - s.layers->opacity;
        const bool retarded = s.t_cross && s.phase_rate != 0.0;
        HIP_TRY(bhg::launch_shade_layers(a, (hipStream_t)s.stream, retarded ? s.t_cross : nullptr, s.phase_rate));
        return BHG_OK;
    }
    HIP_TRY(bhg::launch_shade(a, (hipStream_t)s.stream));
    return BHG_OK;
}

// The mesh shades, bhg_shade_mesh_device and bhg_shade_mesh_material_device, as one call record; shade() above stays what it is.
// The checks, in the order their refusals are seen: the scene; the mesh; the material (the material call only, a NULL one
// refused); the context and its device; n_pixels == 0 is BHG_OK; the device arrays
struct MeshShadeCall {
    ShadeCall s;                              // end, flags, n_pixels, samples, sc, the three outputs and the stream: nothing else is read
    const int32_t *tri_id = nullptr;
    const double *bary = nullptr;             // [n][2]
    const bhg_mesh *mesh = nullptr;
    const float *tri_rgb = nullptr;           // the plain call's colours
    bool material = false;
    const bhg_mesh_material *mat = nullptr;   // the material call's; NULL for the plain call
    // the instanced call (mesh stays NULL: the set's mesh is taken once the set has been checked; mat may be NULL: white)
    const bhg_mesh_instances *instances = nullptr;
    const int32_t *inst_id = nullptr;
    const float *inst_rgb = nullptr;
};

int shade_mesh(bhg_context *c, const MeshShadeCall &call)
{
    MeshShadeCall m = call;
    const ShadeCall &s = m.s;
    BHG_TRY(scene_check(s.sc, s.samples, true));
    if (m.instances) {
        // (the set's mesh pointer is only trusted once the set is known to be this context's and its mesh alive)
        BHG_TRY(bhg::instances_usable(c, m.instances));
        m.mesh = m.instances->mesh;
        m.material = m.mat != nullptr;
    }
    if (!m.mesh) return fail(BHG_E_INVALID, "mesh is NULL");
    if (m.material) {
        BHG_TRY(bhg::mesh_material_check(m.mat, (size_t)m.mesh->view.n_tris, false));
    }
    BHG_TRY(bhg::mesh_on_device_of(c, m.mesh));
    if (s.n_pixels == 0) return BHG_OK;
    if ((!s.rgba && !s.rgba_f32) || !s.end || !s.flags || !s.sc->d_sky || !m.tri_id || !m.bary)
        return fail(BHG_E_INVALID, "NULL device pointer");
    if (m.instances && !m.inst_id) return fail(BHG_E_INVALID, "inst_id is NULL");
    ENTER_DEVICE(c->device);
    bhg::ShadeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.end = s.end;
    a.flags = s.flags;
    a.rgba = s.rgba;
    a.rgba_f32 = s.rgba_f32;
    a.scatter = s.scatter;
    a.n_pixels = s.n_pixels;
    a.samples = s.samples;
    fill_scene_args(a, s.sc);
    if (!m.material && !m.instances) {
        HIP_TRY(bhg::launch_shade_mesh(a, m.mesh->view, m.tri_id, m.bary, m.tri_rgb, (hipStream_t)s.stream));
        return BHG_OK;
    }
    bhg::MeshMaterialArgs ma;
    std::memset(&ma, 0, sizeof(ma));     // (the instanced call without a material: white, no emission)
    if (m.mat) {
        ma.tri_rgb = m.mat->tri_rgb;
        ma.tri_uv = m.mat->tri_uv;
        ma.tri_tex = m.mat->tri_tex;
        for (int j = 0; j < m.mat->n_tex; j++) {
            ma.tex[j] = m.mat->tex[j];
            ma.tex_w[j] = m.mat->tex_w[j];
            ma.tex_h[j] = m.mat->tex_h[j];
        }
        ma.n_tex = m.mat->n_tex;
        ma.emission = m.mat->emission;
    }
    if (m.instances) {
        const hipStream_t st = (hipStream_t)s.stream;
        HIP_TRY(bhg::instances_before_read(m.instances, st));
        if (m.instances->leaf_size && bhg::instance_tree_on())
            HIP_TRY(bhg::launch_shade_mesh_instance_tree(a, m.mesh->view, m.tri_id, m.bary, ma, m.instances->tree, bhg::mesh_culls_on(),
                                                         m.inst_id, m.inst_rgb, st));
        else
            HIP_TRY(bhg::launch_shade_mesh_instances(a, m.mesh->view, m.tri_id, m.bary, ma, m.instances->d_rec, m.instances->n,
                                                     bhg::mesh_culls_on(), m.inst_id, m.inst_rgb, st));
        HIP_TRY(bhg::instances_after_read(m.instances, st));
        return BHG_OK;
    }
    HIP_TRY(bhg::launch_shade_mesh_material(a, m.mesh->view, m.tri_id, m.bary, ma, (hipStream_t)s.stream));
    return BHG_OK;
}

// the scene of the sky-only calls: the sky and nothing else
bhg_scene sky_scene(const float *d_sky, int32_t sky_w, int32_t sky_h)
{
    bhg_scene sc;
    std::memset(&sc, 0, sizeof(sc));
    sc.d_sky = d_sky;
    sc.sky_w = sky_w;
    sc.sky_h = sky_h;
    return sc;
}

}  // namespace

extern "C" {

int bhg_raygen_device(bhg_context *c, int32_t width, int32_t height, int32_t samples, double fov_x, double fov_y,
                      const double *rot9, const double *d_jitter, const int64_t *d_pixels, size_t n_pixels,
                      double *d_k0, void *stream)
{
    return raygen_impl(c, width, height, samples, fov_x, fov_y, rot9, d_jitter, d_pixels, n_pixels, d_k0, stream, nullptr);
}

int bhg_raygen_observer_device(bhg_context *c, const bhg_params *p, const bhg_observer *obs, const double *x0, int32_t width,
                               int32_t height, int32_t samples, double fov_x, double fov_y, const double *rot9,
                               const double *d_jitter, const int64_t *d_pixels, size_t n_pixels, double *d_k0, void *stream)
{
    if (!obs) return bhg_raygen_device(c, width, height, samples, fov_x, fov_y, rot9, d_jitter, d_pixels, n_pixels, d_k0, stream);
    if (!x0) return fail(BHG_E_INVALID, "x0 is NULL (the observer's tetrad depends on the camera position)");
    bhg::ObserverParams op;
    int rc = bhg::observer_params(p, obs, x0, &op);
    if (rc != BHG_OK) return rc;
    return raygen_impl(c, width, height, samples, fov_x, fov_y, rot9, d_jitter, d_pixels, n_pixels, d_k0, stream, &op);
}

int bhg_shade_device(bhg_context *c, const double *d_end, const uint8_t *d_flags, size_t n_pixels, int32_t samples,
                     const float *d_sky, int32_t sky_w, int32_t sky_h, double *d_rgba, void *stream)
{
    const bhg_scene sc = sky_scene(d_sky, sky_w, sky_h);
    return shade(c, {.end = d_end, .flags = d_flags, .n_pixels = n_pixels, .samples = samples, .sc = &sc, .rgba = d_rgba, .stream = stream});
}

int bhg_shade_dir_device(bhg_context *c, const double *d_end_dir, const uint8_t *d_flags, size_t n_pixels, int32_t samples,
                         const float *d_sky, int32_t sky_w, int32_t sky_h, double *d_rgba, float *d_rgba_f32,
                         const int64_t *d_scatter, void *stream)
{
    const bhg_scene sc = sky_scene(d_sky, sky_w, sky_h);
    return shade(c, {.end_dir = d_end_dir, .flags = d_flags, .n_pixels = n_pixels, .samples = samples, .sc = &sc, .rgba = d_rgba,
                     .rgba_f32 = d_rgba_f32, .scatter = d_scatter, .stream = stream});
}

int bhg_shade_scene_device(bhg_context *c, const double *d_end, const uint8_t *d_flags, const int8_t *d_object_id,
                           size_t n_pixels, int32_t samples, const bhg_scene *sc, double *d_rgba, void *stream)
{
    return shade(c, {.end = d_end, .flags = d_flags, .object_id = d_object_id, .n_pixels = n_pixels, .samples = samples, .sc = sc,
                     .rgba = d_rgba, .stream = stream});
}

// the mesh shades (DESIGN.md sections 19 and 20): one call (shade_mesh() above), without and with a material
int bhg_shade_mesh_device(bhg_context *c, const double *d_end, const uint8_t *d_flags, const int32_t *d_tri_id, const double *d_bary,
                          size_t n_pixels, int32_t samples, const bhg_scene *sc, const bhg_mesh *mesh, const float *d_tri_rgb,
                          double *d_rgba, float *d_rgba_f32, const int64_t *d_scatter, void *stream)
{
    return shade_mesh(c, {.s = {.end = d_end, .flags = d_flags, .n_pixels = n_pixels, .samples = samples, .sc = sc, .rgba = d_rgba,
                                .rgba_f32 = d_rgba_f32, .scatter = d_scatter, .stream = stream},
                          .tri_id = d_tri_id, .bary = d_bary, .mesh = mesh, .tri_rgb = d_tri_rgb});
}

int bhg_shade_mesh_material_device(bhg_context *c, const double *d_end, const uint8_t *d_flags, const int32_t *d_tri_id,
                                   const double *d_bary, size_t n_pixels, int32_t samples, const bhg_scene *sc, const bhg_mesh *mesh,
                                   const bhg_mesh_material *mat, double *d_rgba, float *d_rgba_f32, const int64_t *d_scatter,
                                   void *stream)
{
    return shade_mesh(c, {.s = {.end = d_end, .flags = d_flags, .n_pixels = n_pixels, .samples = samples, .sc = sc, .rgba = d_rgba,
                                .rgba_f32 = d_rgba_f32, .scatter = d_scatter, .stream = stream},
                          .tri_id = d_tri_id, .bary = d_bary, .mesh = mesh, .material = true, .mat = mat});
}

// ... over an instance set: mat and d_inst_rgb are optional
int bhg_shade_mesh_instances_device(bhg_context *c, const double *d_end, const uint8_t *d_flags, const int32_t *d_tri_id,
                                    const int32_t *d_inst_id, const double *d_bary, size_t n_pixels, int32_t samples,
                                    const bhg_scene *sc, const bhg_mesh_instances *inst, const bhg_mesh_material *mat,
                                    const float *d_inst_rgb, double *d_rgba, float *d_rgba_f32, const int64_t *d_scatter, void *stream)
{
    if (!inst) return fail(BHG_E_INVALID, "mesh instances: inst is NULL");
    return shade_mesh(c, {.s = {.end = d_end, .flags = d_flags, .n_pixels = n_pixels, .samples = samples, .sc = sc, .rgba = d_rgba,
                                .rgba_f32 = d_rgba_f32, .scatter = d_scatter, .stream = stream},
                          .tri_id = d_tri_id, .bary = d_bary, .mat = mat, .instances = inst, .inst_id = d_inst_id,
                          .inst_rgb = d_inst_rgb});
}

int bhg_shade_scene_f32_device(bhg_context *c, const double *d_end, const uint8_t *d_flags, const int8_t *d_object_id,
                               size_t n_pixels, int32_t samples, const bhg_scene *sc, float *d_rgba_f32,
                               const int64_t *d_scatter, void *stream)
{
    return shade(c, {.end = d_end, .flags = d_flags, .object_id = d_object_id, .n_pixels = n_pixels, .samples = samples, .sc = sc,
                     .rgba_f32 = d_rgba_f32, .scatter = d_scatter, .stream = stream});
}

int bhg_shade_scene_redshift_device(bhg_context *c, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                    const int8_t *d_object_id, size_t n_pixels, int32_t samples, const bhg_scene *sc,
                                    const bhg_params *p, const bhg_redshift *rs, const double *x0_shared, const double *d_k0,
                                    double *d_rgba, float *d_rgba_f32, const int64_t *d_scatter, void *stream)
{
    return shade(c, {.end = d_end, .end_dir = d_end_dir, .flags = d_flags, .object_id = d_object_id, .n_pixels = n_pixels,
                     .samples = samples, .sc = sc, .p = p, .rs = rs, .x0_shared = x0_shared, .k0 = d_k0, .rgba = d_rgba,
                     .rgba_f32 = d_rgba_f32, .scatter = d_scatter, .stream = stream});
}

int bhg_shade_scene_redshift_observer_device(bhg_context *c, const double *d_end, const double *d_end_dir,
                                             const uint8_t *d_flags, const int8_t *d_object_id, size_t n_pixels,
                                             int32_t samples, const bhg_scene *sc, const bhg_params *p,
                                             const bhg_redshift *rs, const bhg_observer *obs, const double *x0_shared,
                                             const double *d_k0, double *d_rgba, float *d_rgba_f32,
                                             const int64_t *d_scatter, void *stream)
{
    return shade(c, {.end = d_end, .end_dir = d_end_dir, .flags = d_flags, .object_id = d_object_id, .n_pixels = n_pixels,
                     .samples = samples, .sc = sc, .p = p, .rs = rs, .obs = obs, .x0_shared = x0_shared, .k0 = d_k0, .rgba = d_rgba,
                     .rgba_f32 = d_rgba_f32, .scatter = d_scatter, .stream = stream});
}

int bhg_shade_scene_textured_device(bhg_context *c, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                    const int8_t *d_object_id, size_t n_pixels, int32_t samples, const bhg_scene *sc,
                                    const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                                    const bhg_object_textures *ot, const double *x0_shared, const double *d_k0, double *d_rgba,
                                    float *d_rgba_f32, const int64_t *d_scatter, void *stream)
{
    return bhg_shade_scene_polarised_device(c, d_end, d_end_dir, d_flags, d_object_id, n_pixels, samples, sc, p, rs, obs, ot,
                                            x0_shared, d_k0, d_rgba, d_rgba_f32, d_scatter, nullptr, nullptr, stream);
}

int bhg_shade_scene_polarised_device(bhg_context *c, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                     const int8_t *d_object_id, size_t n_pixels, int32_t samples, const bhg_scene *sc,
                                     const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                                     const bhg_object_textures *ot, const double *x0_shared, const double *d_k0, double *d_rgba,
                                     float *d_rgba_f32, const int64_t *d_scatter, const bhg_polarisation *pol, double *d_qu,
                                     void *stream)
{
    return bhg_shade_scene_thermal_device(c, d_end, d_end_dir, d_flags, d_object_id, n_pixels, samples, sc, p, rs, obs, ot,
                                          x0_shared, d_k0, d_rgba, d_rgba_f32, d_scatter, pol, d_qu, nullptr, stream);
}

int bhg_shade_scene_thermal_device(bhg_context *c, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                   const int8_t *d_object_id, size_t n_pixels, int32_t samples, const bhg_scene *sc,
                                   const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                                   const bhg_object_textures *ot, const double *x0_shared, const double *d_k0, double *d_rgba,
                                   float *d_rgba_f32, const int64_t *d_scatter, const bhg_polarisation *pol, double *d_qu,
                                   const bhg_disk_thermal *th, void *stream)
{
    return bhg_shade_scene_moving_device(c, d_end, d_end_dir, d_flags, d_object_id, n_pixels, samples, sc, p, rs, obs, ot, x0_shared,
                                         d_k0, d_rgba, d_rgba_f32, d_scatter, pol, d_qu, th, nullptr, stream);
}

int bhg_shade_scene_moving_device(bhg_context *c, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                  const int8_t *d_object_id, size_t n_pixels, int32_t samples, const bhg_scene *sc,
                                  const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                                  const bhg_object_textures *ot, const double *x0_shared, const double *d_k0, double *d_rgba,
                                  float *d_rgba_f32, const int64_t *d_scatter, const bhg_polarisation *pol, double *d_qu,
                                  const bhg_disk_thermal *th, const bhg_object_motion *mo, void *stream)
{
    return shade(c, {.end = d_end, .end_dir = d_end_dir, .flags = d_flags, .object_id = d_object_id, .n_pixels = n_pixels,
                     .samples = samples, .sc = sc, .p = p, .rs = rs, .obs = obs, .ot = ot, .x0_shared = x0_shared, .k0 = d_k0,
                     .rgba = d_rgba, .rgba_f32 = d_rgba_f32, .scatter = d_scatter, .pol = pol, .qu = d_qu, .th = th, .mo = mo,
                     .stream = stream});
}

int bhg_shade_disk_layers_device(bhg_context *c, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                 const double *d_cross, const uint8_t *d_n_cross, size_t n_pixels, int32_t samples,
                                 const bhg_scene *sc, const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                                 const double *x0_shared, const double *d_k0, double *d_rgba, float *d_rgba_f32,
                                 const int64_t *d_scatter, const bhg_disk_thermal *th, const bhg_disk_layers *layers,
                                 void *stream)
{
    return bhg_shade_disk_layers_retarded_device(c, d_end, d_end_dir, d_flags, d_cross, d_n_cross, n_pixels, samples, sc, p, rs, obs,
                                                 x0_shared, d_k0, d_rgba, d_rgba_f32, d_scatter, th, layers, nullptr, 0.0, stream);
}

int bhg_shade_disk_layers_retarded_device(bhg_context *c, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                          const double *d_cross, const uint8_t *d_n_cross, size_t n_pixels, int32_t samples,
                                          const bhg_scene *sc, const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                                          const double *x0_shared, const double *d_k0, double *d_rgba, float *d_rgba_f32,
                                          const int64_t *d_scatter, const bhg_disk_thermal *th, const bhg_disk_layers *layers,
                                          const double *d_t_cross, double phase_rate, void *stream)
{
    if (!std::isfinite(phase_rate)) return fail(BHG_E_INVALID, "phase_rate must be finite");
    // (phase_rate == 0 or no times: the plain layered shade, its own kernels)
    return shade(c, {.end = d_end, .end_dir = d_end_dir, .flags = d_flags, .n_pixels = n_pixels, .samples = samples, .sc = sc, .p = p,
                     .rs = rs, .obs = obs, .x0_shared = x0_shared, .k0 = d_k0, .rgba = d_rgba, .rgba_f32 = d_rgba_f32,
                     .scatter = d_scatter, .th = th, .stream = stream, .layered = true, .cross = d_cross, .n_cross = d_n_cross,
                     .layers = layers, .t_cross = d_t_cross, .phase_rate = phase_rate});
}

int bhg_disk_thermal_device(bhg_context *c, const bhg_params *p, const bhg_disk_thermal *th, const bhg_observer *obs,
                            const double *x0_shared, const double *d_x0, const double *d_k0, const double *d_end,
                            const uint8_t *d_flags, size_t n, double *d_t_em, double *d_rgb, void *stream)
{
    // (the settings are checked before the context: a refusal names its figure with or without a device)
    bhg::ThermalParams tp;
    bhg::RedshiftParams rp;
    BHG_TRY(bhg::thermal_params(p, th, nullptr, nullptr, p && p->disk_r_out > 0.0 ? p->disk_r_in : -1.0, x0_shared, &tp, &rp));
    bhg::ObserverParams op;
    std::memset(&op, 0, sizeof(op));
    if (obs) {
        BHG_TRY(bhg::observer_params(p, obs, x0_shared, &op));
    }
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (!x0_shared == !d_x0) return fail(BHG_E_INVALID, "exactly one of x0_shared / d_x0 must be given");
    if (n == 0) return BHG_OK;
    if (!d_k0 || !d_flags || !d_t_em || !d_rgb) return fail(BHG_E_INVALID, "d_k0 / d_flags / d_t_em / d_rgb is NULL");
    if (n > ((size_t)1 << 39)) return fail(BHG_E_INVALID, "n too large for one launch (at most 2^39 rays)");
    ENTER_DEVICE(c->device);
    bhg::ThermalArgs a;
    std::memset(&a, 0, sizeof(a));
    a.t = tp;
    a.p = rp;
    a.obs = op;
    a.x0 = d_x0;
    a.k0 = d_k0;
    a.end = d_end;
    a.flags = d_flags;
    a.t_em = d_t_em;
    a.rgb = d_rgb;
    a.n = n;
    HIP_TRY(bhg::launch_disk_thermal(a, (hipStream_t)stream));
    return BHG_OK;
}

int bhg_disk_thermal_host(bhg_context *c, const bhg_params *p, const bhg_disk_thermal *th, const bhg_observer *obs,
                          const double *x0, int x0_is_shared, const double *k0, const double *end, const uint8_t *flags, size_t n,
                          double *t_em, double *rgb)
{
    bhg::ThermalParams tp;    // (checked here too, before the context and before any copy)
    bhg::RedshiftParams rp;
    BHG_TRY(bhg::thermal_params(p, th, nullptr, nullptr, p && p->disk_r_out > 0.0 ? p->disk_r_in : -1.0, x0_is_shared ? x0 : nullptr,
                                &tp, &rp));
    if (obs) {
        bhg::ObserverParams chk;
        BHG_TRY(bhg::observer_params(p, obs, x0_is_shared ? x0 : nullptr, &chk));
    }
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (!x0) return fail(BHG_E_INVALID, "x0 is NULL");
    if (n == 0) return BHG_OK;
    if (!k0 || !flags || !t_em || !rgb) return fail(BHG_E_INVALID, "k0 / flags / t_em / rgb is NULL");
    ENTER_DEVICE(c->device);
    const size_t b1 = n * sizeof(double);
    Staged st(c, false);
    const size_t dx = st.in(x0_is_shared ? nullptr : x0, 3 * b1), dk = st.in(k0, 3 * b1), de = st.in(end, 6 * b1),
                 df = st.in(flags, n), dt = st.out(t_em, b1), dc = st.out(rgb, 3 * b1);
    return st.run([&] {
        return bhg_disk_thermal_device(c, p, th, obs, x0_is_shared ? x0 : nullptr, st.at<double>(dx), st.at<double>(dk), st.at<double>(de),
                                       st.at<uint8_t>(df), n, st.at<double>(dt), st.at<double>(dc), c->stream);
    });
}

int bhg_polarisation_device(bhg_context *c, const bhg_params *p, const bhg_polarisation *pol, const bhg_observer *obs,
                            const double *x0_shared, const double *d_x0, const double *d_k0, const double *d_end,
                            const uint8_t *d_flags, size_t n, double *d_evpa, double *d_degree, double *d_mu, void *stream)
{
    // (the settings are checked before the context: a refusal names its figure with or without a device)
    bhg::PolarisationParams pp;
    BHG_TRY(bhg::polarisation_params(p, pol, nullptr, obs, p && p->disk_r_out > 0.0 ? p->disk_r_in : -1.0, x0_shared, &pp));
    if (obs) {
        bhg::ObserverParams chk;
        BHG_TRY(bhg::observer_params(p, obs, x0_shared, &chk));
    }
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (!x0_shared == !d_x0) return fail(BHG_E_INVALID, "exactly one of x0_shared / d_x0 must be given");
    if (n == 0) return BHG_OK;
    if (!d_k0 || !d_flags || !d_evpa || !d_degree) return fail(BHG_E_INVALID, "d_k0 / d_flags / d_evpa / d_degree is NULL");
    if (n > ((size_t)1 << 39)) return fail(BHG_E_INVALID, "n too large for one launch (at most 2^39 rays)");
    ENTER_DEVICE(c->device);
    bhg::PolarisationArgs a;
    std::memset(&a, 0, sizeof(a));
    a.p = pp;
    a.x0 = d_x0;
    a.k0 = d_k0;
    a.end = d_end;
    a.flags = d_flags;
    a.evpa = d_evpa;
    a.degree = d_degree;
    a.mu = d_mu;
    a.n = n;
    HIP_TRY(bhg::launch_polarisation(a, obs != nullptr, (hipStream_t)stream));
    return BHG_OK;
}

int bhg_polarisation_host(bhg_context *c, const bhg_params *p, const bhg_polarisation *pol, const bhg_observer *obs,
                          const double *x0, int x0_is_shared, const double *k0, const double *end, const uint8_t *flags, size_t n,
                          double *evpa, double *degree, double *mu)
{
    bhg::PolarisationParams pp;   // (checked here too, before the context and before any copy)
    BHG_TRY(bhg::polarisation_params(p, pol, nullptr, obs, p && p->disk_r_out > 0.0 ? p->disk_r_in : -1.0, x0_is_shared ? x0 : nullptr,
                                     &pp));
    if (obs) {
        bhg::ObserverParams chk;
        BHG_TRY(bhg::observer_params(p, obs, x0_is_shared ? x0 : nullptr, &chk));
    }
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (!x0) return fail(BHG_E_INVALID, "x0 is NULL");
    if (n == 0) return BHG_OK;
    if (!k0 || !flags || !evpa || !degree) return fail(BHG_E_INVALID, "k0 / flags / evpa / degree is NULL");
    ENTER_DEVICE(c->device);
    const size_t b1 = n * sizeof(double);
    Staged st(c, false);
    const size_t dx = st.in(x0_is_shared ? nullptr : x0, 3 * b1), dk = st.in(k0, 3 * b1), de = st.in(end, 6 * b1),
                 df = st.in(flags, n), dc = st.out(evpa, b1), dd = st.out(degree, b1), dm = st.out(mu, b1);
    return st.run([&] {
        return bhg_polarisation_device(c, p, pol, obs, x0_is_shared ? x0 : nullptr, st.at<double>(dx), st.at<double>(dk), st.at<double>(de),
                                       st.at<uint8_t>(df), n, st.at<double>(dc), st.at<double>(dd), st.at<double>(dm), c->stream);
    });
}

int bhg_redshift_device(bhg_context *c, const bhg_params *p, const bhg_redshift *rs, const double *x0_shared,
                        const double *d_x0, const double *d_k0, const double *d_end, const uint8_t *d_flags, size_t n,
                        double *d_g, void *stream)
{
    return bhg_redshift_observer_device(c, p, rs, nullptr, x0_shared, d_x0, d_k0, d_end, d_flags, n, d_g, stream);
}

int bhg_redshift_observer_device(bhg_context *c, const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                                 const double *x0_shared, const double *d_x0, const double *d_k0, const double *d_end,
                                 const uint8_t *d_flags, size_t n, double *d_g, void *stream)
{
    return bhg_redshift_motion_device(c, p, rs, obs, nullptr, nullptr, 0, x0_shared, d_x0, d_k0, d_end, d_flags, nullptr, n, d_g,
                                      stream);
}

int bhg_redshift_motion_device(bhg_context *c, const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                               const bhg_object_motion *motion, const double *spheres, int32_t n_spheres,
                               const double *x0_shared, const double *d_x0, const double *d_k0, const double *d_end,
                               const uint8_t *d_flags, const int8_t *d_object_id, size_t n, double *d_g, void *stream)
{
    // (the settings are checked before the context: a refusal names its figure with or without a device)
    bhg::RedshiftParams rp;
    BHG_TRY(bhg::redshift_params(p, rs, p && p->disk_r_out > 0.0 ? p->disk_r_in : -1.0, x0_shared, &rp));
    bhg::MotionParams mp;
    std::memset(&mp, 0, sizeof(mp));
    if (motion) {
        if (n_spheres < 0 || n_spheres > BHG_MAX_SPHERES)
            return fail(BHG_E_INVALID, "n_spheres must be in [0, BHG_MAX_SPHERES], not " + std::to_string(n_spheres));
        if (n_spheres > 0 && !spheres) return fail(BHG_E_INVALID, "spheres is NULL");
        BHG_TRY(bhg::motion_params(p, motion, spheres, n_spheres, &mp));
    }
    bhg::ObserverParams op;
    std::memset(&op, 0, sizeof(op));
    if (obs) {
        BHG_TRY(bhg::observer_params(p, obs, x0_shared, &op));
    }
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (!x0_shared == !d_x0) return fail(BHG_E_INVALID, "exactly one of x0_shared / d_x0 must be given");
    if (n == 0) return BHG_OK;
    if (!d_k0 || !d_flags || !d_g) return fail(BHG_E_INVALID, "d_k0 / d_flags / d_g is NULL");
    if (mp.on && !d_object_id) return fail(BHG_E_INVALID, "moving object spheres need d_object_id");
    if (n > ((size_t)1 << 39)) return fail(BHG_E_INVALID, "n too large for one launch (at most 2^39 rays)");
    ENTER_DEVICE(c->device);
    bhg::RedshiftArgs a;
    std::memset(&a, 0, sizeof(a));
    a.p = rp;
    a.x0 = d_x0;
    a.k0 = d_k0;
    a.end = d_end;
    a.flags = d_flags;
    a.g = d_g;
    a.n = n;
    a.obs = op;
    if (mp.on) {
        a.mo = mp;
        a.object_id = d_object_id;
        std::memcpy(a.spheres, spheres, sizeof(double) * 4 * (size_t)n_spheres);
        HIP_TRY(bhg::launch_redshift_motion(a, (hipStream_t)stream));
    } else {
        HIP_TRY(bhg::launch_redshift(a, (hipStream_t)stream));
    }
    return BHG_OK;
}

int bhg_redshift_host(bhg_context *c, const bhg_params *p, const bhg_redshift *rs, const double *x0, int x0_is_shared,
                      const double *k0, const double *end, const uint8_t *flags, size_t n, double *g)
{
    return bhg_redshift_observer_host(c, p, rs, nullptr, x0, x0_is_shared, k0, end, flags, n, g);
}

int bhg_redshift_observer_host(bhg_context *c, const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                               const double *x0, int x0_is_shared, const double *k0, const double *end, const uint8_t *flags,
                               size_t n, double *g)
{
    return bhg_redshift_motion_host(c, p, rs, obs, nullptr, nullptr, 0, x0, x0_is_shared, k0, end, flags, nullptr, n, g);
}

int bhg_redshift_motion_host(bhg_context *c, const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                             const bhg_object_motion *motion, const double *spheres, int32_t n_spheres, const double *x0,
                             int x0_is_shared, const double *k0, const double *end, const uint8_t *flags, const int8_t *object_id,
                             size_t n, double *g)
{
    bhg::RedshiftParams rp;   // (checked here too, before the context and before any copy)
    BHG_TRY(bhg::redshift_params(p, rs, p && p->disk_r_out > 0.0 ? p->disk_r_in : -1.0, x0_is_shared ? x0 : nullptr, &rp));
    bhg::MotionParams mp;
    std::memset(&mp, 0, sizeof(mp));
    if (motion) {
        if (n_spheres < 0 || n_spheres > BHG_MAX_SPHERES)
            return fail(BHG_E_INVALID, "n_spheres must be in [0, BHG_MAX_SPHERES], not " + std::to_string(n_spheres));
        if (n_spheres > 0 && !spheres) return fail(BHG_E_INVALID, "spheres is NULL");
        BHG_TRY(bhg::motion_params(p, motion, spheres, n_spheres, &mp));
    }
    bhg::ObserverParams op;
    if (obs) {
        BHG_TRY(bhg::observer_params(p, obs, x0_is_shared ? x0 : nullptr, &op));
    }
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (!x0) return fail(BHG_E_INVALID, "x0 is NULL");
    if (n == 0) return BHG_OK;
    if (!k0 || !flags || !g) return fail(BHG_E_INVALID, "k0 / flags / g is NULL");
    if (mp.on && !object_id) return fail(BHG_E_INVALID, "moving object spheres need object_id");
    ENTER_DEVICE(c->device);
    const size_t b1 = n * sizeof(double);
    Staged st(c, false);
    const size_t dx = st.in(x0_is_shared ? nullptr : x0, 3 * b1), dk = st.in(k0, 3 * b1), de = st.in(end, 6 * b1),
                 df = st.in(flags, n), dob = st.in(mp.on ? object_id : nullptr, n), dg = st.out(g, b1);
    return st.run([&] {
        return bhg_redshift_motion_device(c, p, rs, obs, motion, spheres, n_spheres, x0_is_shared ? x0 : nullptr, st.at<double>(dx),
                                          st.at<double>(dk), st.at<double>(de), st.at<uint8_t>(df), st.at<int8_t>(dob), n,
                                          st.at<double>(dg), c->stream);
    });
}

int bhg_assemble_frame_f32_device(bhg_context *c, const float *d_slabs, const int64_t *d_index, size_t n_pixels,
                                  float *d_frame, void *stream)
{
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (n_pixels == 0) return BHG_OK;
    if (!d_slabs || !d_index || !d_frame) return fail(BHG_E_INVALID, "NULL device pointer");
    ENTER_DEVICE(c->device);
    HIP_TRY(bhg::launch_gather_rows4(d_slabs, d_index, n_pixels, d_frame, (hipStream_t)stream));
    return BHG_OK;
}

int bhg_trajectory(bhg_context *c, const bhg_params *p, const double *x0, int x0_is_shared, const double *k0, size_t n,
                   uint32_t n_points, double *traj, uint32_t *n_valid, double *end, uint8_t *flags)
{
    return bhg_trajectory_objects(c, p, nullptr, 0, x0, x0_is_shared, k0, n, n_points, traj, n_valid, end, flags, nullptr);
}

int bhg_trajectory_objects(bhg_context *c, const bhg_params *p, const double *spheres, int32_t n_spheres, const double *x0,
                           int x0_is_shared, const double *k0, size_t n, uint32_t n_points, double *traj, uint32_t *n_valid,
                           double *end, uint8_t *flags, int8_t *object_id)
{
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    int rc = validate(p);
    if (rc != BHG_OK) return rc;
    rc = validate_spheres(p, spheres, n_spheres);
    if (rc != BHG_OK) return rc;
    if (n_points < 2) return fail(BHG_E_INVALID, "n_points must be >= 2");
    if (n == 0) return BHG_OK;
    if (!x0 || !k0 || !traj || !n_valid) return fail(BHG_E_INVALID, "x0 / k0 / traj / n_valid is NULL");
    // (the kernels form a ray's byte offsets in 32 bits -- store_result: idx * 48 -- and this call is ONE launch)
    if (n > bhg::BHG_MAX_RAYS_PER_LAUNCH) return fail(BHG_E_INVALID, "bhg_trajectory takes at most 2^26 rays per call");
    ENTER_DEVICE(c->device);
    const size_t in_bytes = n * 3 * sizeof(double) * (x0_is_shared ? 1 : 2);
    const size_t sz_traj = n * 6 * (size_t)n_points * sizeof(double);
    const size_t off_end = sz_traj, off_nv = off_end + n * 6 * sizeof(double), off_steps = off_nv + n * sizeof(uint32_t);
    const size_t off_acc = off_steps + n * sizeof(uint32_t), off_flags = off_acc + n * sizeof(uint32_t);
    const size_t off_obj = off_flags + n;      // [n] int8: the sphere a ray ends on (-1: none); only with spheres
    const bool with_obj = n_spheres > 0;
    rc = ensure(&c->d_in, &c->d_in_bytes, in_bytes);
    if (rc != BHG_OK) return rc;
    rc = ensure(&c->d_out, &c->d_out_bytes, off_obj + n + 64);
    if (rc != BHG_OK) return rc;
    // up to 2048 rays the kernel runs one wave per ray and fills what the ray never reaches with NaN: no memset; the direction
    // of a ONE-ray call (the engine's literal call) rides in the kernel arguments
    const bool wave = bhg::trajectory_wave_per_ray(n);
    const bool one = n == 1 && x0_is_shared;
    double *d_k0 = one ? nullptr : (double *)c->d_in, *d_x0 = x0_is_shared ? nullptr : (double *)c->d_in + n * 3;
    char *o = (char *)c->d_out;
    hipStream_t s = c->stream;
    // Zero-copy samples: a small call (the engine's literal one: one ray, 10,000 samples = 480 kB) whose `traj` is
    // page-locked memory (bhg_host_alloc) has the wave-per-ray kernel write its samples STRAIGHT into the caller's array
    // over PCIe -- no device-to-host copy of the block, no host-side split: 40 of the call's 98 us.  (The kernel's stores
    // are 512-byte runs per sample row; the array is complete when the stream has been waited for.)
    double *d_traj = (double *)o;
    bool direct = false;
    if (wave && sz_traj <= (size_t(4) << 20)) {
        void *dp = nullptr;
        if (is_pinned_range(traj, sz_traj, &dp)) {      // (the WHOLE block, not its first byte: the kernel writes all of it)
            d_traj = (double *)dp;
            direct = true;
        }
    }
    // ... and then the small arrays behind the sample block -- end state, n_valid, counts, flags: at most 2048 rays --
    // are written into the context's page-locked block the same way: the call is a launch and a stream wait, no copy
    char *os = o;     // where the kernel writes those (device address), laid out like the device block from off_end on
    if (direct) {
        rc = ensure_pinned(&c->pin_out, &c->pin_out_bytes, size_t(1) << 20);
        if (rc != BHG_OK) return rc;
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, c->pin_out, 0) == hipSuccess && dp) {
            os = (char *)dp - off_end;
        } else {
            (void)hipGetLastError();
            direct = false;
            d_traj = (double *)o;
        }
    }
    if (d_k0) HIP_TRY(hipMemcpyAsync(d_k0, k0, n * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    if (d_x0) HIP_TRY(hipMemcpyAsync(d_x0, x0, n * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    if (!wave) HIP_TRY(hipMemsetAsync(o, 0xFF, sz_traj, s));  // samples a ray never reaches read back as NaN

    bhg::TraceArgs a;
    std::memset(&a, 0, sizeof(a));
    a.k0 = d_k0;
    a.x0 = d_x0;
    a.end = (double *)(os + off_end);
    if (one) {
        a.k0s[0] = k0[0];
        a.k0s[1] = k0[1];
        a.k0s[2] = k0[2];
    }
    a.flags = (uint8_t *)(os + off_flags);
    a.n_steps = (uint32_t *)(os + off_steps);
    a.n_accepted = (uint32_t *)(os + off_acc);
    a.counter = c->counter;        // (the trajectory kernel hands out no batches)
    a.counter_next = nullptr;
    a.n = n;
    if (!d_x0) {
        a.x0s[0] = x0[0];
        a.x0s[1] = x0[1];
        a.x0s[2] = x0[2];
    }
    const int rhs_id = fill_trace_args(a, p, spheres, n_spheres);
    a.min_step_cap = 0.0;
    a.object_id = with_obj ? (int8_t *)(os + off_obj) : nullptr;
    HIP_TRY(bhg::launch_trajectory(a, rhs_id, p->method, d_traj, (uint32_t *)(os + off_nv), n_points, s));
    const size_t total = with_obj ? off_obj + n : off_flags + n;
    if (object_id && !with_obj) std::memset(object_id, 0xFF, n);      // (no spheres: no ray ends on one)
    if (direct) {
        const char *h = (const char *)c->pin_out - off_end;
        // (polling hipStreamQuery before the blocking wait was measured: no gain, the runtime already spins)
        HIP_TRY(hipStreamSynchronize(s));
        std::memcpy(n_valid, h + off_nv, n * sizeof(uint32_t));
        if (end) std::memcpy(end, h + off_end, n * 6 * sizeof(double));
        if (flags) std::memcpy(flags, h + off_flags, n);
        if (object_id && with_obj) std::memcpy(object_id, h + off_obj, n);
        return BHG_OK;
    }
    if (total <= (size_t(4) << 20)) {
        // the engine's per-ray call (one ray, 10,000 samples: 480 kB): ONE copy of the whole output block into page-locked
        // memory and a host-side split, instead of four copies into the caller's pageable arrays (each of which the
        // runtime stages and waits for on its own)
        rc = ensure_pinned(&c->pin_out, &c->pin_out_bytes, total < (size_t(1) << 20) ? (size_t(1) << 20) : (size_t(4) << 20));
        if (rc != BHG_OK) return rc;
        const char *h = (const char *)c->pin_out;
        HIP_TRY(hipMemcpyAsync(c->pin_out, o, total, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::memcpy(traj, h, sz_traj);
        std::memcpy(n_valid, h + off_nv, n * sizeof(uint32_t));
        if (end) std::memcpy(end, h + off_end, n * 6 * sizeof(double));
        if (flags) std::memcpy(flags, h + off_flags, n);
        if (object_id && with_obj) std::memcpy(object_id, h + off_obj, n);
        return BHG_OK;
    }
    HIP_TRY(hipMemcpyAsync(traj, o, sz_traj, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(n_valid, o + off_nv, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (end) HIP_TRY(hipMemcpyAsync(end, o + off_end, n * 6 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (flags) HIP_TRY(hipMemcpyAsync(flags, o + off_flags, n, hipMemcpyDeviceToHost, s));
    if (object_id && with_obj) HIP_TRY(hipMemcpyAsync(object_id, o + off_obj, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return BHG_OK;
}

int bhg_acceleration(bhg_context *c, const bhg_params *p, const double *x, const double *k, size_t n, double *acc)
{
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    BHG_TRY(validate(p));
    if (n == 0) return BHG_OK;
    if (!x || !k || !acc) return fail(BHG_E_INVALID, "x / k / acc is NULL");
    ENTER_DEVICE(c->device);
    BHG_TRY(ensure(&c->d_in, &c->d_in_bytes, n * 6 * sizeof(double)));
    BHG_TRY(ensure(&c->d_out, &c->d_out_bytes, n * 3 * sizeof(double)));
    double *dx = (double *)c->d_in, *dk = dx + 3 * n;
    HIP_TRY(hipMemcpyAsync(dx, x, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dk, k, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(bhg::launch_accel(dx, dk, p->r_s, p->spin, p->time_like ? 1.0 : 0.0, n, (double *)c->d_out,
                              (p->time_like && p->rhs_form == BHG_RHS_CHRISTOFFEL) ? bhg::BHG_RHS_CHRISTOFFEL_TL_ : p->rhs_form, c->stream));
    HIP_TRY(hipMemcpyAsync(acc, c->d_out, n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BHG_OK;
}

int bhg_peak_probe(bhg_context *c, int32_t kind, double target_ms, double out[6])
{
    if (!c || !out) return fail(BHG_E_INVALID, "bad argument");
    if (kind != BHG_PROBE_FMA && kind != BHG_PROBE_STEP_MIX) return fail(BHG_E_INVALID, "unknown probe kind");
    if (!(target_ms >= 0.0) || target_ms > 100.0) return fail(BHG_E_INVALID, "target_ms must be in [0, 100] (0 = 1 ms)");
    if (target_ms == 0.0) target_ms = 1.0;
    ENTER_DEVICE(c->device);
    const int per_cu = 12;                       // the Schwarzschild trace kernels' residency (3 waves per SIMD)
    const int grid = per_cu * c->num_cus;
    BHG_TRY(ensure(&c->d_out, &c->d_out_bytes, (size_t)grid * 64 * sizeof(double)));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    hipError_t he = hipEventCreate(&e1);
    if (he != hipSuccess) {
        (void)hipEventDestroy(e0);
        return fail_hip(he, "hipEventCreate");
    }
    auto timed = [&](uint32_t iters, float *ms) -> hipError_t {
        hipError_t e = hipEventRecord(e0, c->stream);
        if (e == hipSuccess) e = bhg::launch_probe(kind, grid, iters, (double *)c->d_out, c->stream);
        if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(ms, e0, e1);
        return e;
    };
    // size the loop for the asked duration from a short launch, then take the median of five
    uint32_t iters = 64;
    float ms = 0.0f;
    he = timed(iters, &ms);
    if (he == hipSuccess) he = timed(iters, &ms);
    float runs[5] = {0, 0, 0, 0, 0};
    if (he == hipSuccess) {
        const double scale = target_ms / std::fmax((double)ms, 1e-3);
        iters = (uint32_t)std::fmin(std::fmax(64.0 * scale, 16.0), 4.0e6);
        he = timed(iters, &ms);   // (one untimed launch at the final size)
        for (int i = 0; i < 5 && he == hipSuccess; i++) he = timed(iters, &runs[i]);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (he != hipSuccess) return fail_hip(he, "bhg_peak_probe");
    std::sort(runs, runs + 5);
    uint32_t valu = 0, quarter = 0;
    bhg::probe_shape(kind, &valu, &quarter);
    const double waves = (double)grid;
    const double wave_insts = waves * (double)iters * (double)valu;
    // flops under SURVEY section 8d's counting rule: an FMA is 2, a reciprocal / reciprocal square root 1
    const double flops = waves * 64.0 * (double)iters * (2.0 * (double)(valu - quarter) + (double)quarter);
    const double sec = (double)runs[2] * 1e-3;
    out[0] = flops / sec * 1e-12;
    out[1] = (double)runs[2];
    out[2] = wave_insts;
    out[3] = waves * (double)iters * (double)quarter;
    out[4] = (double)runs[0];
    // the clock a full-rate fp64 pipe (128 flop per clock and CU) would need for that figure: for the pure-FMA probe the
    // sustained shader clock itself
    out[5] = out[0] * 1e12 / (128.0 * (double)c->num_cus) * 1e-6;
    return BHG_OK;
}

int bhg_math_probe(bhg_context *c, int32_t op, const double *in, size_t n, double *out)
{
    // (the refusals come before the context, as everywhere: a test needs no device for them)
    int n_in = 0, n_out = 0;
    if (!bhg::math_probe_shape(op, &n_in, &n_out)) return fail(BHG_E_INVALID, "unknown math probe op " + std::to_string(op));
    if (n > 0 && (!in || !out)) return fail(BHG_E_INVALID, "math probe: in / out is NULL");
    if (n > ((size_t)1 << 26)) return fail(BHG_E_INVALID, "math probe: at most 2^26 elements per call");
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (n == 0) return BHG_OK;
    ENTER_DEVICE(c->device);
    BHG_TRY(ensure(&c->d_in, &c->d_in_bytes, n * (size_t)n_in * sizeof(double)));
    BHG_TRY(ensure(&c->d_out, &c->d_out_bytes, n * (size_t)n_out * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(c->d_in, in, n * (size_t)n_in * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(bhg::launch_math_probe(op, (const double *)c->d_in, n, (double *)c->d_out, c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->d_out, n * (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BHG_OK;
}

}  // extern "C"
