// ikpso_api.cpp -- the C ABI (include/ikpso.h): validation, solver handles,
// dispatch to the gfx950 kernels.  The chain parser is ikpso_chain.cpp.
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <new>
#include <vector>

#include "ikpso.h"
#include "ikpso_chain.h"
#include "ikpso_kernels.h"

using namespace ikpso;

// csrc/_build/ikpso_build_id.cpp, written by the Makefile on every build
extern "C" const char ikpso_build_id_string[];

static_assert(sizeof(ikpso_node) == 88, "ikpso_node must match NodeCUDA (88 bytes)");
static_assert(sizeof(ikpso_rng_state) == 48, "ikpso_rng_state must match curandStateXORWOW (48 bytes)");
static_assert(sizeof(ikpso_pso_config) == 16, "PSOConfig is 16 bytes");
static_assert(sizeof(ikpso_fitness_config) == 12, "FitnessConfig is 12 bytes");
static_assert(sizeof(ikpso_collider) == 48, "obj_t is 48 bytes");

// Collider-term counters of an IKPSO_COLLIDE_STATS build (tools/collide_stats.py):
// one device block for the process, read and cleared by ikpso_debug_collide_stats.
unsigned long long* ikpso::collide_stats_buffer()
{
#if IKPSO_COLLIDE_STATS
    static unsigned long long* buf = nullptr;
    if (!buf && hipMalloc(&buf, kCsCount * sizeof(unsigned long long)) == hipSuccess)
        (void)hipMemset(buf, 0, kCsCount * sizeof(unsigned long long));
    return buf;
#else
    return nullptr;
#endif
}

#if IKPSO_COLLIDE_STATS
// [kCsCount] counters since the last reset (reset != 0 clears them after the read).
extern "C" int ikpso_debug_collide_stats(unsigned long long* out, int reset)
{
    unsigned long long* buf = ikpso::collide_stats_buffer();
    if (!buf) return (int)hipErrorMemoryAllocation;
    hipError_t e = hipMemcpy(out, buf, ikpso::kCsCount * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e == hipSuccess && reset) e = hipMemset(buf, 0, ikpso::kCsCount * sizeof(unsigned long long));
    return (int)e;
}
#endif

namespace {

thread_local int g_last_hip_error = 0;
std::atomic<int64_t> g_coop_fallbacks{0};  // cooperative solves re-run on the streaming kernels

ikpso_status hip_status(hipError_t e)
{
    if (e == hipSuccess) return IKPSO_OK;
    g_last_hip_error = (int)e;
    return e == hipErrorOutOfMemory ? IKPSO_ERR_NO_MEMORY : IKPSO_ERR_HIP;
}

#define IKPSO_HIP(call)                                  \
    do {                                                 \
        hipError_t e_ = (call);                          \
        if (e_ != hipSuccess) return hip_status(e_);     \
    } while (0)

// Copy `bytes` from host, managed or device memory into host memory.
// Pageable host memory (what a caller's plain arrays are; the Python mirror's
// numpy tables) is copied on the CPU: nothing on the GPU can be writing it, and
// the per-frame node table then costs no device round trip.  Pinned host,
// device and managed memory go through hipMemcpy, which orders the read after
// the caller's queued GPU work (an async copy that fills a pinned buffer, or a
// kernel writing the managed node table).
ikpso_status fetch_any(void* dst, const void* src, size_t bytes)
{
    if (bytes == 0) return IKPSO_OK;
    // hipPointerGetAttributes reports an unregistered host pointer as an error and
    // records it as the thread's last error: clear it (the entry points have taken
    // any error the caller's own earlier work left, take_pending_error)
    hipPointerAttribute_t a{};
    const hipError_t e = hipPointerGetAttributes(&a, src);
    if (e != hipSuccess) (void)hipGetLastError();
    if (e != hipSuccess || a.type == hipMemoryTypeUnregistered) {
        memcpy(dst, src, bytes);
        return IKPSO_OK;
    }
    IKPSO_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDefault));
    return IKPSO_OK;
}

// An error the caller's earlier HIP work left pending (not yet read by
// hipGetLastError) is reported up front by the next entry point that runs HIP
// work (calculate_pso, solver_create, solve_batch), which then leaves every buffer
// and the solver state untouched.  The reference's calculatePSO also returns such
// an error, from its first cudaGetLastError check (src/kernel.cu:293-295), but only
// after its init kernels have already rewritten particles, bests and randoms.
// Taking it here also keeps it from being mistaken for a launch failure of this
// call (the launches are checked with hipGetLastError) and from being cleared by
// fetch_any / is_device_memory, which clear the errors their own lookups cause.
hipError_t take_pending_error() { return hipGetLastError(); }

// Host copies of a scene's arrays (each from host, managed or device memory) and the
// Extras that point into them.  The optional arrays are null where the entry point
// has none; `positions` is null unless the distance term reads it.
struct SceneHost {
    std::vector<ikpso_node> nodes;
    std::vector<uint8_t> mask;
    std::vector<float> pos, slo, shi;
    std::vector<ikpso_collider> boxes;
    Extras ex;

    ikpso_status fetch(const ikpso_node* chain, int node_count, const float* positions, bool posref_node_slot,
                       const ikpso_collider* colliders, int collider_count, const uint8_t* axis_mask = nullptr,
                       float limit_weight = 0.0f, const float* soft_lo = nullptr, const float* soft_hi = nullptr)
    {
        const int J = node_count - 1;
        nodes.resize(node_count);
        ikpso_status st = fetch_any(nodes.data(), chain, sizeof(ikpso_node) * node_count);
        if (st != IKPSO_OK) return st;
        int D = 3 * J;  // free dimensions
        if (axis_mask) {
            mask.resize(node_count);
            if ((st = fetch_any(mask.data(), axis_mask, mask.size())) != IKPSO_OK) return st;
            ex.axis_mask = mask.data();
            D = 0;
            for (int k = 1; k <= J; ++k) D += __builtin_popcount(mask[k] & 7u);
        }
        if (positions) {
            ex.posref_node_slot = posref_node_slot;
            pos.resize(4 * (size_t)(posref_node_slot ? J + 2 : J));
            if ((st = fetch_any(pos.data(), positions, sizeof(float) * pos.size())) != IKPSO_OK) return st;
            ex.positions = pos.data();
        }
        if (limit_weight != 0.0f) {
            if (!soft_lo || !soft_hi) return IKPSO_ERR_INVALID_ARG;
            slo.resize(D);
            shi.resize(D);
            if ((st = fetch_any(slo.data(), soft_lo, sizeof(float) * D)) != IKPSO_OK) return st;
            if ((st = fetch_any(shi.data(), soft_hi, sizeof(float) * D)) != IKPSO_OK) return st;
            ex.limit_weight = limit_weight;
            ex.soft_lo = slo.data();
            ex.soft_hi = shi.data();
        }
        if (collider_count < 0 || (collider_count > 0 && !colliders)) return IKPSO_ERR_INVALID_ARG;
        if (collider_count > 0) {
            boxes.resize(collider_count);
            if ((st = fetch_any(boxes.data(), colliders, sizeof(ikpso_collider) * boxes.size())) != IKPSO_OK)
                return st;
            ex.colliders = boxes.data();
            ex.collider_count = collider_count;
        }
        return IKPSO_OK;
    }
};

// Grow a device array to hold at least `need` items of `unit` bytes (contents not kept).
template <class T, class N>
ikpso_status grow(T** buf, N* have, N need, size_t unit)
{
    if (need <= *have) return IKPSO_OK;
    if (*buf) IKPSO_HIP(hipFree(*buf));  // hipFree synchronises the device
    *buf = nullptr;
    *have = 0;
    IKPSO_HIP(hipMalloc(reinterpret_cast<void**>(buf), (size_t)need * unit));
    *have = need;
    return IKPSO_OK;
}

// A coherent, mapped pinned block of `words` int32 (a kernel writes it, the host reads
// it after one synchronisation): its host address and the device's.
ikpso_status pinned_words(size_t words, int32_t** host, int32_t** dev)
{
    void* h = nullptr;
    IKPSO_HIP(hipHostMalloc(&h, sizeof(int32_t) * words, hipHostMallocCoherent | hipHostMallocMapped));
    void* dv = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&dv, h, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(h);
        IKPSO_HIP(e);
    }
    *host = static_cast<int32_t*>(h);
    *dev = static_cast<int32_t*>(dv);
    return IKPSO_OK;
}

// Device scratch of the reference-compatible path (result staging, aux terms,
// streaming workspace).  The entry point holds g_scratch_mu for its whole call.
std::mutex g_scratch_mu;
float* g_scratch = nullptr;
size_t g_scratch_bytes = 0;

// What the per-frame call keeps between frames (under g_scratch_mu), so that a
// frame's device work is the solve kernel alone (round 4: the aux upload, the
// generator snapshot copy, the slot clear and two small D2H copies were 4 extra
// dependent operations of ~20 us around a 57 us kernel, profiles/r04/frame_*):
//  * aux: the last uploaded aux block and where it lies; a frame re-uploads only
//    when its content or place changed (the scene's bounds do not, per frame);
//  * slots: the cooperative slot region left by the last frame (CoopSlotState);
//  * pinned: [error flag | answer], written by the kernels themselves (coherent
//    pinned memory, read after the call's one synchronisation).
// A cooperative workspace's slot region between launches: [at, at + bytes)
// holds only zeros or granules tagged below `next`, so a launch there numbers
// its exchanges from `next` (SwarmIO::coop_tag0) instead of clearing the slots.
struct CoopSlotState {
    char* at = nullptr;
    size_t bytes = 0;
    uint32_t next = 0;
    void invalidate() { bytes = 0; }  // something else was written over the region
    // `exchanges`: an upper bound on the exchanges one group of the launch runs.
    hipError_t begin(SwarmIO& io, char* ws, size_t zero, uint64_t exchanges, hipStream_t s)
    {
        if (at != ws || zero > bytes || exchanges >= 0x7FFFFFFFull || (uint64_t)next + exchanges + 1 >= 0xFFFFFFFFull) {
            const hipError_t e = hipMemsetAsync(ws, 0, zero, s);
            if (e != hipSuccess) return e;
            next = 0;
        }
        io.coop_tag0 = next;
        next = exchanges >= 0x7FFFFFFFull ? 0xFFFFFFFFu : next + (uint32_t)exchanges + 1;  // (cleared next time)
        at = ws;
        bytes = zero;  // what lies past it (the snapshot, the fallback's workspace) is not known clean
        return hipSuccess;
    }
};

struct CompatFrameCache {
    const float* aux_at = nullptr;
    std::vector<float> aux;
    CoopSlotState slots;
    int32_t* pinned = nullptr;      // host address
    int32_t* pinned_dev = nullptr;  // its device address
};
CompatFrameCache g_frame;
constexpr size_t kFramePinnedWords = 64 + 3 * kMaxJoints;  // the flag, then the answer at word 64

ikpso_status scratch(size_t bytes, float** out)
{
    const size_t had = g_scratch_bytes;
    const ikpso_status st = grow(&g_scratch, &g_scratch_bytes, bytes, 1);
    if (g_scratch_bytes != had) {
        g_frame.aux_at = nullptr;  // nothing of the old block is known to survive
        g_frame.slots.invalidate();
    }
    *out = g_scratch;
    return st;
}

// True when `p` is memory of the current device (a kernel writes it directly;
// anything else -- pageable, pinned or managed host memory, another GPU's memory --
// gets the answer through the pinned block and a copy).
bool is_device_memory(const void* p)
{
    hipPointerAttribute_t a{};
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) (void)hipGetLastError();  // our own lookup's error (see fetch_any)
    int cur = -1;
    return e == hipSuccess && a.type == hipMemoryTypeDevice && hipGetDevice(&cur) == hipSuccess && a.device == cur;
}

// Carve 256-byte aligned arrays out of one allocation.
struct Carver {
    char* base;
    size_t off = 0;
    template <class T>
    T* take(size_t n)
    {
        off = (off + 255) & ~size_t(255);
        T* p = reinterpret_cast<T*>(base + off);
        off += n * sizeof(T);
        return p;
    }
};

// Streaming workspace layout (see StreamIO); state/pbf carved only when not
// supplied by the caller.
void carve_stream(StreamIO& io, void* ws, int64_t B, int P, int D, bool own_state)
{
    Carver cv{static_cast<char*>(ws)};
    const int C = (P + kStreamChunk - 1) / kStreamChunk;
    if (own_state) {
        io.state = cv.take<float>((size_t)B * 3 * D * P);
        io.pbf = cv.take<float>((size_t)B * P);
    }
    io.rng = cv.take<uint32_t>((size_t)6 * B * P);
    io.pkey = cv.take<uint32_t>((size_t)2 * B * C);
    io.pidx = cv.take<int32_t>((size_t)2 * B * C);
    io.pvec = cv.take<float>((size_t)2 * B * C * D);
    io.gkey = cv.take<uint32_t>((size_t)2 * B);
    io.gidx = cv.take<int32_t>((size_t)2 * B);
    io.gvec = cv.take<float>((size_t)2 * B * D);
    io.iters = cv.take<int32_t>((size_t)B);
    io.num_swarms = B;
    io.P = P;
    io.C = C;
}

int env_kernel()
{
    const char* e = getenv("IKPSO_KERNEL");
    if (!e) return IKPSO_KERNEL_AUTO;
    if (strcmp(e, "resident") == 0) return IKPSO_KERNEL_RESIDENT;
    if (strcmp(e, "streaming") == 0) return IKPSO_KERNEL_STREAMING;
    if (strcmp(e, "coop") == 0) return IKPSO_KERNEL_COOP;
    return IKPSO_KERNEL_AUTO;
}

// Cooperative launch plan for B swarms of P particles: chunk size (the
// throughput block, or with `latency` the 256-lane block when every swarm then
// still gets its own CUs), G chunks per swarm, NG concurrent groups (a
// multiple of 8 for the XCD-aware membership, kCoopBlocksPerCU workgroups per CU, at most
// ceil8(B)).  False if infeasible.
// linear (only with `allow_linear`): a latency group wider than an XCD (G > CUs / 8:
// the visualiser's N = 16384 is 64 chunks) spans XCDs with linear membership (group =
// workgroup / G, NG = CUs / G, not a multiple of 8); its hand-offs cross XCDs (agent-scope
// granules are coherent there, MI355X_MICROARCH: +0.1-0.3 us per hop).
struct CoopPlan {
    int G = 0, NG = 0, block = 0;
    bool linear = false;
    // the latency variant runs (long chains' throughput chunks are kCoopLatencyThreads wide
    // too: only a block other than the throughput one is the latency plan)
    bool latency = false;
};

bool coop_plan(const ChainHost& ch, int P, int64_t B, bool latency, bool allow_linear, CoopPlan* plan)
{
    CoopGeometry geo;
    if (!coop_geometry(ch, &geo)) return false;
    int T = geo.threads;
    *plan = CoopPlan{};
    if (latency && geo.latency_variant) {
        const int gl = (P + kCoopLatencyThreads - 1) / kCoopLatencyThreads;
        if (gl <= 64 && B * gl <= (int64_t)geo.cus && ((geo.cus / gl) & ~7) >= 8) T = kCoopLatencyThreads;
        if (allow_linear && T != kCoopLatencyThreads && gl <= 64 && B * gl <= (int64_t)geo.cus &&
            coop_latency_split(ch)) {
            *plan = {gl, (int)std::min<int64_t>(B, geo.cus / gl), kCoopLatencyThreads, true, true};
            return true;
        }
    }
    const int g = (P + T - 1) / T;
    int ng = (geo.cus * geo.blocks_per_cu / g) & ~7;
    if (g > 64 || ng < 8) return false;
    const int64_t want = ((B + 7) / 8) * 8;
    if (want < ng) ng = (int)want;
    *plan = {g, ng, T, false, T != geo.threads};
    return true;
}

// AUTO for a swarm that fits one workgroup: the latency variant of the
// cooperative kernel when every swarm gets its own CUs (a few swarms: more
// CUs per swarm), else the resident kernel.
bool prefer_latency_coop(const ChainHost& ch, int P, int64_t B)
{
    CoopPlan plan;
    return coop_plan(ch, P, B, true, false, &plan) && plan.block == kCoopLatencyThreads;
}

// Bound on a cooperative group wait (IKPSO_COOP_SPIN_LIMIT: debug knob; 0
// forces the give-up path so the fallback can be tested).
uint32_t coop_spin_limit()
{
    // only an explicit decimal number overrides the default: an empty or
    // malformed value (which strtoul would read as 0, the give-up path) is ignored
    const char* e = getenv("IKPSO_COOP_SPIN_LIMIT");
    if (!e || !*e) return kCoopSpinLimit;
    char* end = nullptr;
    const unsigned long v = strtoul(e, &end, 10);
    if (end == e || *end != '\0' || v > 0xFFFFFFFFul) return kCoopSpinLimit;
    return (uint32_t)v;
}

// Point the coop fields of `io` into workspace `ws` (coop_workspace_bytes).
// *zero_bytes: the extent of the flag + slots from `ws`, which start at 0 (tags
// are exchange numbers + 1) or hold tags below io.coop_tag0 + 1.
hipError_t carve_coop(SwarmIO& io, void* ws, const CoopPlan& plan, int D, hipStream_t s, size_t* zero_bytes)
{
    const int G = plan.G, NG = plan.NG;
    io.coop_tag0 = 0;
    io.coop_spin_limit = coop_spin_limit();
    io.coop_linear = plan.linear ? 1 : 0;
    Carver cv{static_cast<char*>(ws)};
    io.coop_error = cv.take<int32_t>(1);
    io.coop_slots = cv.take<unsigned long long>((size_t)NG * 2 * G * kCoopSlot(D));
    io.coop_timing = IKPSO_COOP_TIMING ? cv.take<unsigned long long>((size_t)NG * G * 8) : nullptr;
    io.coop_g = G;
    io.coop_ng = NG;
    io.coop_block = plan.block;
    *zero_bytes = reinterpret_cast<char*>(io.coop_slots + (size_t)NG * 2 * G * kCoopSlot(D)) - static_cast<char*>(ws);
    return IKPSO_COOP_TIMING ? hipMemsetAsync(io.coop_timing, 0, (size_t)NG * G * 64, s) : hipSuccess;
}

// Set a cooperative launch up in workspace `ws`: carve it, number the launch's
// exchanges past the tags the slots hold (`exchanges` bounds those one group runs;
// CoopSlotState::begin clears the slots instead when it must), and have the kernel
// raise its error flag in pinned memory, at device address `flag_dev`.
hipError_t begin_coop(SwarmIO& io, CoopSlotState& slots, void* ws, const CoopPlan& plan, int D, uint64_t exchanges,
                      int32_t* flag_dev, hipStream_t s)
{
    size_t zero = 0;
    hipError_t e = carve_coop(io, ws, plan, D, s, &zero);
    if (e == hipSuccess) e = slots.begin(io, static_cast<char*>(ws), zero, exchanges, s);
    io.coop_error = flag_dev;
    return e;
}

// Resolve the kernel family for a chain and swarm size; -1 if impossible.
int pick_kernel(const ChainHost& ch, int P, int requested)
{
    const bool fits = P <= resident_max_threads(ch);
    CoopPlan plan;
    const bool coop = coop_plan(ch, P, 1, false, false, &plan);
    if (requested == IKPSO_KERNEL_RESIDENT) return fits ? IKPSO_KERNEL_RESIDENT : -1;
    if (requested == IKPSO_KERNEL_STREAMING) return IKPSO_KERNEL_STREAMING;
    if (requested == IKPSO_KERNEL_COOP) return coop ? IKPSO_KERNEL_COOP : -1;
    return fits ? IKPSO_KERNEL_RESIDENT : (coop ? IKPSO_KERNEL_COOP : IKPSO_KERNEL_STREAMING);
}

// The term a track entry adds to every fitness, and so the track kernels it runs: the folded chain's pose
// kernels (ikpso_solve_track_pose) or aim kernels (ikpso_solve_track_aim), or the Euler topologies'
// effector-frame kernels (ikpso_solve_track_frames).  None: the plain track kernel.
struct TrackTerm {
    enum Kind { kNone, kPose, kAim, kFrames };
    Kind kind = kNone;
    bool weighted = false;  // the weight, or some effector's, is > 0 (solve_track_term)
    // the targets on the device: kPose [frames][B][9] rotations, kAim [frames][B][3] directions,
    // kFrames [frames][B][E][9] rotations per effector
    const float* target = nullptr;
    float weight = 0.0f;                  // kPose, kAim
    float aim_axis[3] = {};               // kAim: a' = G a (aim_axis_folded)
    float eff_rot_w[kMaxEffFrames] = {};  // kFrames: the caller's weight per effector
};

// What one solve launches with (the arguments of the solve entry points).
struct SolveArgs {
    const float* targets = nullptr;
    const float* start_pose = nullptr;
    int64_t num_swarms = 0;
    int32_t iterations = 0;
    float *out_angles = nullptr, *out_fitness = nullptr, *out_residual = nullptr;
    uint32_t stop_key = 0;              // ikpso_solve_batch_until (0: no stop)
    int32_t* out_iterations = nullptr;
    int32_t frames = 0;  // > 0: ikpso_solve_track, every buffer but start_pose time-major
    TrackTerm term;      // ikpso_solve_track_pose, _aim, _frames: the term's track kernels
};

// The kernels the last solve ran, for ikpso_solver_kernel_name.
enum Route {
    kRouteOwn,      // the solver's own family
    kRouteStream,   // the streaming kernels solve_batch_until runs for an AUTO cooperative solver
    kRouteLatency,  // the cooperative latency variant AUTO may pick per call
    // A resident AUTO solver of a long chain (256-lane chunks: no separate latency build) still
    // takes the cooperative route for a swarm of one chunk: the name reported is that kernel's.
    kRouteCoop,
    kRouteFrames,  // the resident track kernels with the effector rotation term (ikpso_solve_track_frames)
    kRouteCount
};

}  // namespace

struct ikpso_solver {
    ChainHost chain;       // the node table as given (Euler form, with its axis mask)
    float* aux = nullptr;  // device copy of chain.aux
    // The folded form (TopoDH) a FAST solver of a masked serial chain solves with;
    // evaluate and REFERENCE solves use `chain`.
    ChainHost dhchain;
    bool use_dh = false;
    float* aux_dh = nullptr;
    const ChainHost& solve_chain() const { return use_dh ? dhchain : chain; }
    int family = IKPSO_KERNEL_RESIDENT;
    int requested = IKPSO_KERNEL_AUTO;
    std::string kname[kRouteCount];  // kernel family / topology of each route
    Route last = kRouteOwn;
    void* ws = nullptr;    // streaming / cooperative workspace
    size_t ws_bytes = 0;
    int P = 0;
    int mode = IKPSO_ARITH_FAST;
    ikpso_rng_state* rng = nullptr;
    int64_t capacity = 0;
    // Cooperative solves: the generator states as they were before the launch,
    // and what ikpso_solver_sync needs to re-run the batch on the streaming
    // kernels if a group could not assemble.
    ikpso_rng_state* rng_snap = nullptr;
    int64_t snap_capacity = 0;
    struct {
        bool active = false;
        SolveArgs args;
        hipStream_t stream = nullptr;
    } pending;
    int64_t fallbacks = 0;
    // a cooperative solve's error flag, in coherent pinned memory the kernel writes
    // (read by ikpso_solver_sync after its synchronisation), and its device address
    int32_t* err_host = nullptr;
    int32_t* err_dev = nullptr;
    CoopSlotState slots;  // the cooperative slots in `ws` between solves
#if IKPSO_COOP_TIMING
    unsigned long long* pending_timing = nullptr;
    int pending_timing_n = 0;
#endif
};

namespace {

// Free whatever a solver holds, half-built or complete (nothing may still run on it).
void free_solver(ikpso_solver* s)
{
    if (s->rng) (void)hipFree(s->rng);
    if (s->rng_snap) (void)hipFree(s->rng_snap);
    if (s->err_host) (void)hipHostFree(s->err_host);
    if (s->aux) (void)hipFree(s->aux);
    if (s->aux_dh) (void)hipFree(s->aux_dh);
    if (s->ws) (void)hipFree(s->ws);
    delete s;
}

// The resident and cooperative kernels' block for a solve of `s`.
SwarmIO swarm_io(const ikpso_solver* s, const SolveArgs& a)
{
    SwarmIO io{};
    io.frames = a.frames;
    io.targets = a.targets;
    io.start_pose = a.start_pose;
    io.rng = s->rng;
    io.out_angles = a.out_angles;
    io.out_fitness = a.out_fitness;
    io.out_residual = a.out_residual;
    io.P = s->P;
    io.iterations = a.iterations;
    io.num_swarms = a.num_swarms;
    io.stop_key = a.stop_key;
    io.out_iterations = a.out_iterations;
    for (int i = 0; i < 9; ++i) io.tip_rot[i] = s->solve_chain().tip_rot[i];
    const TrackTerm& t = a.term;
    switch (t.kind) {  // (the routing ints: launch_resident)
    case TrackTerm::kNone: break;
    case TrackTerm::kPose:
        io.pose = 1;
        io.target_rot = t.target;
        io.orient_w = t.weight;
        break;
    case TrackTerm::kAim:
        io.aim = 1;
        io.aim_dir = t.target;
        io.aim_w = t.weight;
        for (int i = 0; i < 3; ++i) io.aim_axis[i] = t.aim_axis[i];
        break;
    case TrackTerm::kFrames:
        io.eff_frames = 1;
        io.eff_rot = t.target;
        for (int i = 0; i < kMaxEffFrames; ++i) io.eff_rot_w[i] = t.eff_rot_w[i];
        break;
    }
    return io;
}

// The batch on the streaming kernels (state in HBM, I + 2 launches; no
// co-residency requirement), in the solver's workspace, grown as needed.
ikpso_status solve_streaming(ikpso_solver* s, const SolveArgs& a, hipStream_t hs)
{
    const ChainHost& ch = s->solve_chain();
    const int D = ch.kernel_dims();
    s->slots.invalidate();  // the streaming workspace overwrites the cooperative slots
    ikpso_status st = grow(&s->ws, &s->ws_bytes, stream_workspace_bytes(a.num_swarms, s->P, D, true), 1);
    if (st != IKPSO_OK) return st;
    StreamIO io{};
    carve_stream(io, s->ws, a.num_swarms, s->P, D, true);
    io.rng_aos = s->rng;
    io.targets = a.targets;
    io.start_pose = a.start_pose;
    io.out_angles = a.out_angles;
    io.out_fitness = a.out_fitness;
    io.out_residual = a.out_residual;
    io.stop_key = a.stop_key;
    io.out_iterations = a.out_iterations;
    IKPSO_HIP(launch_stream(ch, s->mode, io, a.iterations, hs));
    return IKPSO_OK;
}

// The batch on the resident kernel: one launch, one workgroup per swarm.
ikpso_status solve_resident(ikpso_solver* s, const SolveArgs& a, hipStream_t hs)
{
    IKPSO_HIP(launch_resident(s->solve_chain(), s->mode, swarm_io(s, a), hs));
    return IKPSO_OK;
}

// The batch on the cooperative kernel: one launch, left pending for ikpso_solver_sync.
ikpso_status solve_coop(ikpso_solver* s, const SolveArgs& a, hipStream_t hs)
{
    const ChainHost& ch = s->solve_chain();
    const int D = ch.kernel_dims();
    const int64_t B = a.num_swarms;
    CoopPlan plan;
    if (!coop_plan(ch, s->P, B, s->requested == IKPSO_KERNEL_AUTO, true, &plan)) return IKPSO_ERR_UNSUPPORTED;
    const size_t had = s->ws_bytes;
    ikpso_status st = grow(&s->ws, &s->ws_bytes, coop_workspace_bytes(plan.NG, plan.G, D), 1);
    if (st != IKPSO_OK) return st;
    if (s->ws_bytes != had) s->slots.invalidate();  // a new allocation: contents unknown
    if (!s->err_host && (st = pinned_words(1, &s->err_host, &s->err_dev)) != IKPSO_OK) return st;
    // snapshot of the generator states the launch starts from (48 B per
    // particle): the fallback re-runs the batch from it.  One swarm: the kernel
    // writes it as its chunks load the states; more: one D2D copy before the
    // launch (a group that gives up never loads its later swarms)
    const size_t swarm_bytes = sizeof(ikpso_rng_state) * (size_t)s->P;
    if (B > s->snap_capacity && (st = grow(&s->rng_snap, &s->snap_capacity, s->capacity, swarm_bytes)) != IKPSO_OK)
        return st;
    if (B > 1) IKPSO_HIP(hipMemcpyAsync(s->rng_snap, s->rng, swarm_bytes * B, hipMemcpyDeviceToDevice, hs));
    SwarmIO io = swarm_io(s, a);
    io.rng_snap = B == 1 ? s->rng_snap : nullptr;
    // a group runs at most every swarm: B (I + 1) exchanges bound its numbering
    IKPSO_HIP(begin_coop(io, s->slots, s->ws, plan, D, (uint64_t)B * ((uint64_t)a.iterations + 1), s->err_dev, hs));
    *s->err_host = 0;  // the previous solve has settled: nothing writes it now
    s->last = plan.latency ? kRouteLatency : kRouteCoop;  // the reported name follows the variant that runs
    IKPSO_HIP(launch_coop(ch, s->mode, io, hs));
    s->pending.active = true;
    s->pending.args = a;
    s->pending.stream = hs;
#if IKPSO_COOP_TIMING
    s->pending_timing = io.coop_timing;
    s->pending_timing_n = plan.NG * plan.G;
#endif
    return IKPSO_OK;
}

// What the solve entries share once their own argument checks have passed: the
// checks against the seeded capacity, an error the caller left pending, the previous
// cooperative solve if it was not synced, and the route bookkeeping.  `stops`: the
// entry needs a kernel that can stop a swarm early, which the cooperative ones cannot.
ikpso_status begin_solve(ikpso_solver* s, int64_t num_swarms, bool stops)
{
    if (num_swarms > s->capacity || !s->rng) return IKPSO_ERR_INVALID_ARG;  // seed first
    if (num_swarms > 0x7fffffff) return IKPSO_ERR_INVALID_ARG;
    if (stops && s->requested == IKPSO_KERNEL_COOP) return IKPSO_ERR_UNSUPPORTED;
    IKPSO_HIP(take_pending_error());
    if (s->pending.active) {  // settle it first
        const ikpso_status st = ikpso_solver_sync(s);
        if (st != IKPSO_OK) return st;
    }
    s->last = stops && s->family != IKPSO_KERNEL_RESIDENT ? kRouteStream : kRouteOwn;
    return IKPSO_OK;
}

// ikpso_solve_batch_until's threshold as the kernels compare it (negative: never stop)
uint32_t stop_key_of(float stop_fitness) { return stop_fitness < 0.0f ? 0u : ordered_key_host(stop_fitness); }

// The caller's weight per effector (rot_weights: E host values, or null for every weight 0) into the
// kernels' kMaxEffFrames slots.  False: a weight is NaN, negative or infinite.  *any: some weight is > 0,
// one beyond the slots included.
bool effector_weights(const float* rot_weights, int E, float (&slots)[kMaxEffFrames], bool* any)
{
    *any = false;
    for (int e = 0; rot_weights && e < E; ++e) {
        const float w = rot_weights[e];
        if (!(w >= 0.0f) || w > FLT_MAX) return false;
        if (e < kMaxEffFrames) slots[e] = w;
        *any = *any || w > 0.0f;
    }
    return true;
}

// What ikpso_solver_evaluate_frames and ikpso_solver_evaluate_gradient check alike: the solver, the count,
// the angles and the entry's required outputs (outputs_ok), then the weights into rot_w, then that a
// weight > 0 -- or an output that reads the targets whatever the weights (reads_target) -- has target_rot.
bool rot_term_args(const ikpso_solver* s, const float* angles, int64_t n, bool outputs_ok, const float* rot_weights,
                   const float* target_rot, bool reads_target, float (&rot_w)[kMaxEffFrames])
{
    if (!s || n < 0 || (n > 0 && (!angles || !outputs_ok))) return false;
    bool weighted = false;
    if (!effector_weights(rot_weights, s->chain.E, rot_w, &weighted)) return false;
    return target_rot || !(weighted || reads_target);
}

// What the four track entries share, and the order of their answers (DESIGN, "The track entries' status
// ladder"): every invalid argument, the common ones here and then the entry's own; a solver the entry does
// not serve; the empty call; then begin_solve and the launch.  term_checks(term) is the entry's part: it
// fills the term in and returns IKPSO_ERR_INVALID_ARG, or IKPSO_ERR_UNSUPPORTED when nothing else is
// wrong but the solver has no kernel with the term, or IKPSO_OK.
// The frame loop of ikpso_solve_batch_until calls in one call.  Resident family: one launch, the loop
// inside the kernel (swarm_track_body).  Streaming (the plain entry alone; also for a solver AUTO routed
// to the cooperative family, as in solve_batch_until): the loop here, one streaming solve per frame over
// pointer offsets, so the contract holds by construction.
template <class TermChecks>
ikpso_status solve_track_term(ikpso_solver* s, const float* targets, const float* start_pose, int64_t num_swarms,
                              int32_t frames, int32_t max_iterations, float stop_fitness, float* out_angles,
                              float* out_fitness, float* out_residual, int32_t* out_iterations, void* stream,
                              TermChecks&& term_checks)
{
    if (!s || num_swarms < 0 || frames < 0 || max_iterations < 0 || stop_fitness != stop_fitness)
        return IKPSO_ERR_INVALID_ARG;
    if (frames > 0 && (!targets || !out_angles)) return IKPSO_ERR_INVALID_ARG;
    SolveArgs all{targets,     start_pose,   num_swarms,           max_iterations, out_angles,
                  out_fitness, out_residual, stop_key_of(stop_fitness), out_iterations, frames};
    ikpso_status st = term_checks(all.term);
    if (st != IKPSO_OK) return st;
    if (num_swarms == 0 || frames == 0) return IKPSO_OK;
    if ((st = begin_solve(s, num_swarms, true)) != IKPSO_OK) return st;
    // Weight 0 (every weight 0) is the term absent: the plain track kernel computes that fitness, and only
    // it gives ikpso_solve_track's bits.  A term's kernel evaluates the same position expressions, but the
    // compiler contracts an a*b + c*d of them into an FMA the other way round here and there (the kernels'
    // contraction is not pinned), an ulp away.
    if (!all.term.weighted) all.term = TrackTerm{};
    if (all.term.kind == TrackTerm::kFrames) s->last = kRouteFrames;
    const hipStream_t hs = (hipStream_t)stream;
    if (s->last != kRouteStream) return solve_resident(s, all, hs);
    const int64_t B = num_swarms, nt = B * s->chain.E * 3, na = B * s->chain.dof();  // one frame of targets, of angles
    for (int64_t t = 0; t < frames && st == IKPSO_OK; ++t) {
        SolveArgs a = all;
        a.frames = 0;
        a.targets = targets + t * nt;
        a.start_pose = t ? out_angles + (t - 1) * na : start_pose;
        a.out_angles = out_angles + t * na;
        if (out_fitness) a.out_fitness = out_fitness + t * B;
        if (out_residual) a.out_residual = out_residual + t * B;
        if (out_iterations) a.out_iterations = out_iterations + t * B;
        st = solve_streaming(s, a, hs);
    }
    return st;
}

}  // namespace

extern "C" {

int ikpso_abi_version(void) { return IKPSO_ABI_VERSION; }

const char* ikpso_build_id(void) { return ikpso_build_id_string; }

int ikpso_last_hip_error(void) { return g_last_hip_error; }

const char* ikpso_status_string(ikpso_status s)
{
    switch (s) {
    case IKPSO_OK: return "ok";
    case IKPSO_ERR_INVALID_ARG: return "invalid argument";
    case IKPSO_ERR_UNSUPPORTED: return "unsupported configuration";
    case IKPSO_ERR_HIP: return "HIP runtime error";
    case IKPSO_ERR_NO_MEMORY: return "out of device memory";
    default: return "unknown status";
    }
}

ikpso_status ikpso_init_generators_seeded(ikpso_rng_state* randoms, int64_t count, uint64_t seed_base, void* stream)
{
    if (count < 0 || (count > 0 && !randoms)) return IKPSO_ERR_INVALID_ARG;
    IKPSO_HIP(launch_init_generators(randoms, count, seed_base, (hipStream_t)stream));
    return IKPSO_OK;
}

// initGenerators (src/utility_kernels.cuh:33-47): launch, then synchronise.
ikpso_status ikpso_init_generators(ikpso_rng_state* randoms, int size, void* stream)
{
    ikpso_status s = ikpso_init_generators_seeded(randoms, size, 0, stream);
    if (s != IKPSO_OK) return s;
    IKPSO_HIP(hipStreamSynchronize((hipStream_t)stream));
    return IKPSO_OK;
}

ikpso_status ikpso_calculate_pso(float* particles, const float* positions, float* bests, ikpso_rng_state* randoms,
                                 int size, const ikpso_node* chain, int node_count, ikpso_pso_config pso,
                                 ikpso_fitness_config fit, float* result, const ikpso_collider* colliders,
                                 int collider_count, void* stream)
{
    if (collider_count < 0 || (collider_count > 0 && !colliders)) return IKPSO_ERR_INVALID_ARG;
    if (size <= 0 || !particles || !bests || !randoms || !chain || !result || node_count < 2 ||
        node_count - 1 > kMaxJoints || pso.iterations < 0)
        return IKPSO_ERR_INVALID_ARG;
    IKPSO_HIP(take_pending_error());
    const bool use_pos = fit.distance_weight != 0.0f && positions;
    const char* ps = use_pos ? getenv("IKPSO_POSREF") : nullptr;
    SceneHost sc;
    ikpso_status st = sc.fetch(chain, node_count, use_pos ? positions : nullptr, ps && strcmp(ps, "node_slot") == 0,
                               colliders, collider_count);
    if (st != IKPSO_OK) return st;
    const int D = 3 * (node_count - 1);
    ChainHost ch;
    st = parse_chain(sc.nodes, pso, fit, sc.ex, ch);
    if (st != IKPSO_OK) return st;
    // The reference-compatible entry has no mode argument; IKPSO_ARITH=reference
    // selects the reference's operation order (parity runs).
    const char* env = getenv("IKPSO_ARITH");
    const int mode = (env && strcmp(env, "reference") == 0) ? IKPSO_ARITH_REFERENCE : IKPSO_ARITH_FAST;
    const int family = pick_kernel(ch, size, env_kernel());
    if (family < 0) return IKPSO_ERR_UNSUPPORTED;
    int family_run = family;
    if (family == IKPSO_KERNEL_RESIDENT && env_kernel() == IKPSO_KERNEL_AUTO && prefer_latency_coop(ch, size, 1))
        family_run = IKPSO_KERNEL_COOP;
    CoopPlan plan;
    if (family_run == IKPSO_KERNEL_COOP && !coop_plan(ch, size, 1, env_kernel() == IKPSO_KERNEL_AUTO, true, &plan))
        return IKPSO_ERR_UNSUPPORTED;

    std::lock_guard<std::mutex> lk(g_scratch_mu);
    // device scratch: [aux (at float ceil64(D)) | workspace]; aux is uploaded here (when
    // it changed) and the call synchronises before returning, so `ch.aux` outlives
    // every use.  The cooperative path also keeps a snapshot of the generator
    // states (written by the kernel as it loads them) and room for the streaming
    // fallback.  The answer goes to `result` directly when that is device memory,
    // else to the pinned block, copied out after the synchronisation.
    const size_t aux_at = ((size_t)D + 63) & ~size_t(63);
    const size_t head = sizeof(float) * (aux_at + ch.aux.size());
    const size_t sws = stream_workspace_bytes(1, size, D, false);
    const size_t snap = ((sizeof(ikpso_rng_state) * (size_t)size + 255) & ~size_t(255));
    const size_t cws = family_run == IKPSO_KERNEL_COOP ? ((coop_workspace_bytes(plan.NG, plan.G, D) + 255) & ~size_t(255)) : 0;
    const size_t ws = family_run == IKPSO_KERNEL_STREAMING ? sws
                      : family_run == IKPSO_KERNEL_COOP ? cws + snap + sws
                                                          : 0;
    float* dres = nullptr;
    st = scratch(((head + 255) & ~size_t(255)) + ws, &dres);
    if (st != IKPSO_OK) return st;
    if (!g_frame.pinned && (st = pinned_words(kFramePinnedWords, &g_frame.pinned, &g_frame.pinned_dev)) != IKPSO_OK)
        return st;
    const bool direct = is_device_memory(result);
    float* const out = direct ? result : reinterpret_cast<float*>(g_frame.pinned_dev + 64);
    const hipStream_t s = (hipStream_t)stream;
    // the cached block is compared byte for byte (a value comparison would take -0 for +0 and
    // never match a NaN)
    if (g_frame.aux_at != dres + aux_at || g_frame.aux.size() != ch.aux.size() ||
        (!ch.aux.empty() && memcmp(g_frame.aux.data(), ch.aux.data(), sizeof(float) * ch.aux.size()) != 0)) {
        IKPSO_HIP(hipMemcpyAsync(dres + aux_at, ch.aux.data(), sizeof(float) * ch.aux.size(), hipMemcpyHostToDevice, s));
        g_frame.aux_at = dres + aux_at;
        g_frame.aux = ch.aux;
    }
    ch.aux_dev = dres + aux_at;
    char* const wsb = reinterpret_cast<char*>(dres) + ((head + 255) & ~size_t(255));
    if (family_run != IKPSO_KERNEL_COOP) g_frame.slots.invalidate();  // the streaming workspace overwrites the slots
    // the streaming kernels with their workspace at `at`: the reference's own [3][D][P]
    // layout is the streaming state
    const auto stream_solve = [&](void* at) {
        StreamIO io{};
        carve_stream(io, at, 1, size, D, false);
        io.state = particles;
        io.pbf = bests;
        io.rng_aos = randoms;
        io.out_angles = out;
        return launch_stream(ch, mode, io, pso.iterations, s);
    };
    ikpso_rng_state* const rsnap = reinterpret_cast<ikpso_rng_state*>(wsb + cws);
    if (family_run == IKPSO_KERNEL_STREAMING) {
        IKPSO_HIP(stream_solve(wsb));
    } else {
        SwarmIO io{};
        io.rng = randoms;
        io.out_angles = out;
        io.dump_particles = particles;
        io.dump_bests = bests;
        io.P = size;
        io.iterations = pso.iterations;
        io.num_swarms = 1;
        if (family_run == IKPSO_KERNEL_RESIDENT) {
            IKPSO_HIP(launch_resident(ch, mode, io, s));
        } else {
            io.rng_snap = rsnap;  // one swarm, started by its group: the snapshot is complete
            // one swarm: I + 1 exchanges
            IKPSO_HIP(begin_coop(io, g_frame.slots, wsb, plan, D, (uint64_t)pso.iterations + 1, g_frame.pinned_dev, s));
            __atomic_store_n(g_frame.pinned, 0, __ATOMIC_RELEASE);
            IKPSO_HIP(launch_coop(ch, mode, io, s));
        }
    }
    IKPSO_HIP(hipStreamSynchronize(s));
    if (family_run == IKPSO_KERNEL_COOP && __atomic_load_n(g_frame.pinned, __ATOMIC_ACQUIRE) != 0) {
        // The group could not assemble (other work held CUs): restore the
        // generator states and solve on the streaming kernels, which need
        // no co-residency -- the caller never sees the contention.
        IKPSO_HIP(hipMemcpyAsync(randoms, rsnap, sizeof(ikpso_rng_state) * (size_t)size, hipMemcpyDeviceToDevice, s));
        IKPSO_HIP(stream_solve(reinterpret_cast<char*>(rsnap) + snap));
        g_coop_fallbacks.fetch_add(1);
        IKPSO_HIP(hipStreamSynchronize(s));
    }
    if (!direct) memcpy(result, g_frame.pinned + 64, sizeof(float) * D);
    return IKPSO_OK;
}

ikpso_status ikpso_solver_create(const ikpso_solver_desc* desc, ikpso_solver** out)
{
    if (!desc || !out || !desc->chain || desc->node_count < 2 || desc->node_count - 1 > kMaxJoints ||
        desc->particles <= 0)
        return IKPSO_ERR_INVALID_ARG;
    if (desc->arith != IKPSO_ARITH_FAST && desc->arith != IKPSO_ARITH_REFERENCE) return IKPSO_ERR_INVALID_ARG;
    *out = nullptr;
    // a caller's pending error is reported here, before fetch_any's own lookups
    // (which clear the errors they cause) could discard it
    IKPSO_HIP(take_pending_error());
    SceneHost sc;
    const bool use_pos = desc->fit.distance_weight != 0.0f && desc->positions;
    ikpso_status st = sc.fetch(desc->chain, desc->node_count, use_pos ? desc->positions : nullptr,
                               (desc->flags & IKPSO_FLAG_POSREF_NODE_SLOT) != 0, desc->colliders, desc->collider_count,
                               desc->axis_mask, desc->limit_weight, desc->soft_lo, desc->soft_hi);
    if (st != IKPSO_OK) return st;
    ikpso_solver* s = new (std::nothrow) ikpso_solver();
    if (!s) return IKPSO_ERR_NO_MEMORY;
    const auto fail = [s](ikpso_status why) {
        free_solver(s);
        return why;
    };
    if ((st = parse_chain(sc.nodes, desc->pso, desc->fit, sc.ex, s->chain)) != IKPSO_OK) return fail(st);
    s->P = desc->particles;
    s->mode = desc->arith;
    // FAST solves of a masked serial chain run on its folded form
    s->use_dh = s->mode == IKPSO_ARITH_FAST && !(desc->flags & IKPSO_FLAG_NO_FOLD) &&
                build_dh(sc.nodes, s->chain, sc.ex, s->dhchain);
    const auto upload = [](float** dev, const std::vector<float>& host) {
        const size_t bytes = sizeof(float) * host.size();
        const hipError_t e = hipMalloc(dev, bytes);
        return e == hipSuccess ? hipMemcpy(*dev, host.data(), bytes, hipMemcpyHostToDevice) : e;
    };
    // the Euler chain's aux with the kept colliders' indices behind it (ChainHost::coll_index)
    std::vector<float> aux_idx = s->chain.aux;
    aux_idx.resize(s->chain.aux.size() + s->chain.coll_index.size());
    for (size_t j = 0; j < s->chain.coll_index.size(); ++j) {
        const int32_t index = s->chain.coll_index[j];
        memcpy(&aux_idx[s->chain.aux.size() + j], &index, sizeof(index));
    }
    hipError_t e = upload(&s->aux, aux_idx);
    if (e == hipSuccess && s->use_dh) e = upload(&s->aux_dh, s->dhchain.aux);
    if (e != hipSuccess) return fail(hip_status(e));
    s->chain.aux_dev = s->aux;
    s->dhchain.aux_dev = s->aux_dh;
    const ChainHost& sch = s->solve_chain();
    s->family = pick_kernel(sch, s->P, desc->kernel);
    s->requested = desc->kernel;
    if (s->family < 0 || desc->kernel < IKPSO_KERNEL_AUTO || desc->kernel > IKPSO_KERNEL_COOP)
        return fail((desc->kernel == IKPSO_KERNEL_RESIDENT || desc->kernel == IKPSO_KERNEL_COOP) ? IKPSO_ERR_UNSUPPORTED
                                                                                                  : IKPSO_ERR_INVALID_ARG);
    s->kname[kRouteOwn] = kernel_name(sch, s->family);
    s->kname[kRouteStream] = kernel_name(sch, IKPSO_KERNEL_STREAMING);
    s->kname[kRouteCoop] = kernel_name(sch, IKPSO_KERNEL_COOP);
    s->kname[kRouteFrames] = kernel_name(sch, IKPSO_KERNEL_RESIDENT).insert(strlen("swarm_resident"), "_frames");
    s->kname[kRouteLatency] = s->kname[kRouteCoop] +
                              (coop_latency_split(sch) ? " (latency variant, generator waves)" : " (latency variant)");
    *out = s;
    return IKPSO_OK;
}

ikpso_status ikpso_solver_destroy(ikpso_solver* s)
{
    if (!s) return IKPSO_OK;
    // a pending cooperative solve still runs on the buffers freed below: settle it
    // (its fallback, if it needs one, completes the caller's outputs)
    const ikpso_status pend = s->pending.active ? ikpso_solver_sync(s) : IKPSO_OK;
    free_solver(s);
    return pend;
}

ikpso_status ikpso_solver_seed(ikpso_solver* s, int64_t capacity, uint64_t seed_base, int64_t first_swarm,
                               void* stream)
{
    if (!s || capacity < 0 || first_swarm < 0) return IKPSO_ERR_INVALID_ARG;
    if (s->pending.active) {  // settle the last cooperative solve before its states are replaced
        const ikpso_status st = ikpso_solver_sync(s);
        if (st != IKPSO_OK) return st;
    }
    const ikpso_status st = grow(&s->rng, &s->capacity, capacity, sizeof(ikpso_rng_state) * (size_t)s->P);
    if (st != IKPSO_OK) return st;
    IKPSO_HIP(launch_init_generators(s->rng, capacity * s->P, seed_base + (uint64_t)first_swarm * s->P,
                                     (hipStream_t)stream));
    return IKPSO_OK;
}

ikpso_status ikpso_solve_batch(ikpso_solver* s, const float* targets, const float* start_pose, int64_t num_swarms,
                               int32_t iterations, float* out_angles, float* out_fitness, float* out_residual,
                               void* stream)
{
    if (!s || num_swarms < 0 || iterations < 0) return IKPSO_ERR_INVALID_ARG;
    if (num_swarms == 0) return IKPSO_OK;
    if (!out_angles) return IKPSO_ERR_INVALID_ARG;  // targets == NULL: chain targets for every swarm
    const ikpso_status st = begin_solve(s, num_swarms, false);
    if (st != IKPSO_OK) return st;
    const SolveArgs a{targets, start_pose, num_swarms, iterations, out_angles, out_fitness, out_residual};
    const hipStream_t hs = (hipStream_t)stream;
    const bool latency_coop = s->family == IKPSO_KERNEL_RESIDENT && s->requested == IKPSO_KERNEL_AUTO &&
                              prefer_latency_coop(s->solve_chain(), s->P, num_swarms);
    if (latency_coop) s->last = kRouteLatency;
    if (s->family == IKPSO_KERNEL_COOP || latency_coop) return solve_coop(s, a, hs);
    return s->family == IKPSO_KERNEL_RESIDENT ? solve_resident(s, a, hs) : solve_streaming(s, a, hs);
}

// The cooperative kernels draw the next iteration's first dimensions inside the
// exchange that would decide whether that iteration runs, so they have no stop: a
// solver AUTO routed to them runs the streaming kernels here, and a resident solver
// never takes the few-swarm cooperative latency route.
ikpso_status ikpso_solve_batch_until(ikpso_solver* s, const float* targets, const float* start_pose,
                                     int64_t num_swarms, int32_t max_iterations, float stop_fitness,
                                     float* out_angles, float* out_fitness, float* out_residual,
                                     int32_t* out_iterations, void* stream)
{
    if (!s || num_swarms < 0 || max_iterations < 0 || stop_fitness != stop_fitness) return IKPSO_ERR_INVALID_ARG;
    if (num_swarms == 0) return IKPSO_OK;
    if (!out_angles) return IKPSO_ERR_INVALID_ARG;
    const ikpso_status st = begin_solve(s, num_swarms, true);
    if (st != IKPSO_OK) return st;
    const SolveArgs a{targets,     start_pose,   num_swarms,           max_iterations, out_angles,
                      out_fitness, out_residual, stop_key_of(stop_fitness), out_iterations};
    return s->last == kRouteStream ? solve_streaming(s, a, (hipStream_t)stream)
                                   : solve_resident(s, a, (hipStream_t)stream);
}

ikpso_status ikpso_solve_track(ikpso_solver* s, const float* targets, const float* start_pose, int64_t num_swarms,
                               int32_t frames, int32_t max_iterations, float stop_fitness, float* out_angles,
                               float* out_fitness, float* out_residual, int32_t* out_iterations, void* stream)
{
    return solve_track_term(s, targets, start_pose, num_swarms, frames, max_iterations, stop_fitness, out_angles,
                            out_fitness, out_residual, out_iterations, stream,
                            [](TrackTerm&) { return IKPSO_OK; });
}

// ikpso_solve_track on the folded chain's pose kernels: the same frame loop in one launch, the
// orientation term in every fitness.  No other kernel has the term, so no other solver is served.
ikpso_status ikpso_solve_track_pose(ikpso_solver* s, const float* targets, const float* target_rot,
                                    float orientation_weight, const float* start_pose, int64_t num_swarms,
                                    int32_t frames, int32_t max_iterations, float stop_fitness, float* out_angles,
                                    float* out_fitness, float* out_residual, int32_t* out_iterations, void* stream)
{
    return solve_track_term(s, targets, start_pose, num_swarms, frames, max_iterations, stop_fitness, out_angles,
                            out_fitness, out_residual, out_iterations, stream, [&](TrackTerm& term) {
        if (!(orientation_weight >= 0.0f)) return IKPSO_ERR_INVALID_ARG;  // negative or NaN
        if (orientation_weight > 0.0f && !target_rot) return IKPSO_ERR_INVALID_ARG;
        term.kind = TrackTerm::kPose;
        term.weighted = orientation_weight > 0.0f;
        term.target = target_rot;
        term.weight = orientation_weight;
        return s->use_dh && s->family == IKPSO_KERNEL_RESIDENT ? IKPSO_OK : IKPSO_ERR_UNSUPPORTED;
    });
}

// ikpso_solve_track on the folded chain's aim kernels: the pose entry's routing and refusals, the
// tool-axis term |R_eff a - d|^2 in the orientation term's place.
ikpso_status ikpso_solve_track_aim(ikpso_solver* s, const float* targets, const float* aim_dir, const float* aim_axis,
                                   float aim_weight, const float* start_pose, int64_t num_swarms, int32_t frames,
                                   int32_t max_iterations, float stop_fitness, float* out_angles, float* out_fitness,
                                   float* out_residual, int32_t* out_iterations, void* stream)
{
    return solve_track_term(s, targets, start_pose, num_swarms, frames, max_iterations, stop_fitness, out_angles,
                            out_fitness, out_residual, out_iterations, stream, [&](TrackTerm& term) {
        if (!(aim_weight >= 0.0f)) return IKPSO_ERR_INVALID_ARG;  // negative or NaN
        if (aim_weight > 0.0f && (!aim_dir || !aim_axis)) return IKPSO_ERR_INVALID_ARG;
        term.kind = TrackTerm::kAim;
        term.weighted = aim_weight > 0.0f;
        if (term.weighted && !aim_axis_folded(s->solve_chain(), aim_axis, term.aim_axis)) return IKPSO_ERR_INVALID_ARG;
        term.target = aim_dir;
        term.weight = aim_weight;
        return s->use_dh && s->family == IKPSO_KERNEL_RESIDENT ? IKPSO_OK : IKPSO_ERR_UNSUPPORTED;
    });
}

// ikpso_solve_track on the Euler topologies' effector-frame kernels: the same frame loop in one launch,
// a rotation term per effector in every fitness.  Only the FAST runtime-term track build without mask or
// collider block has the term, so only the solvers that build can serve are served.
ikpso_status ikpso_solve_track_frames(ikpso_solver* s, const float* targets, const float* target_rot,
                                      const float* rot_weights, const float* start_pose, int64_t num_swarms,
                                      int32_t frames, int32_t max_iterations, float stop_fitness, float* out_angles,
                                      float* out_fitness, float* out_residual, int32_t* out_iterations, void* stream)
{
    return solve_track_term(s, targets, start_pose, num_swarms, frames, max_iterations, stop_fitness, out_angles,
                            out_fitness, out_residual, out_iterations, stream, [&](TrackTerm& term) {
        const ChainHost& ch = s->chain;
        term.kind = TrackTerm::kFrames;
        if (!effector_weights(rot_weights, ch.E, term.eff_rot_w, &term.weighted)) return IKPSO_ERR_INVALID_ARG;
        if (term.weighted && !target_rot) return IKPSO_ERR_INVALID_ARG;
        term.target = target_rot;
        // the refusal ladder: REFERENCE arithmetic; any axis mask (folded, or kept by IKPSO_FLAG_NO_FOLD); a
        // collider term the kernels test (or their polynomial sin/cos); another family than the resident one
        const bool served = s->mode == IKPSO_ARITH_FAST && !s->use_dh && !ch.masked && ch.num_coll == 0 &&
                            !ch.poly_trig && s->family == IKPSO_KERNEL_RESIDENT && ch.E <= kMaxEffFrames;
        return served ? IKPSO_OK : IKPSO_ERR_UNSUPPORTED;
    });
}

// ordered_key_host / key_to_float, for the tests (not part of the declared ABI)
uint32_t ikpso_debug_ordered_key(float f) { return ordered_key_host(f); }
float ikpso_debug_key_to_float(uint32_t k) { return key_to_float_host(k); }

ikpso_status ikpso_solver_sync(ikpso_solver* s)
{
    if (!s) return IKPSO_ERR_INVALID_ARG;
    if (!s->pending.active) return IKPSO_OK;
    auto& p = s->pending;
    // `pending` stays active until the flag has been read and, if a group gave
    // up, the fallback has run: a failure on the way (an allocation, a copy)
    // returns its error and leaves the solve pending, so the next sync, solve or
    // generator_states call settles it instead of reporting OK over NaN answers.
    // the kernel writes the flag into coherent pinned memory: one synchronisation
    IKPSO_HIP(hipStreamSynchronize(p.stream));
    const int32_t err = __atomic_load_n(s->err_host, __ATOMIC_ACQUIRE);
#if IKPSO_COOP_TIMING
    if (s->pending_timing) {  // measurement build: mean cycles per iteration over the workgroups
        std::vector<unsigned long long> t((size_t)s->pending_timing_n * 8);
        IKPSO_HIP(hipMemcpy(t.data(), s->pending_timing, t.size() * 8, hipMemcpyDeviceToHost));
        double a = 0, b = 0, c = 0, it = 0, imp = 0, rem = 0, pol = 0, ah = 0;
        for (size_t i = 0; i < t.size(); i += 8)
            a += t[i], b += t[i + 1], it += t[i + 2], c += t[i + 3], imp += t[i + 4], rem += t[i + 5],
                pol += t[i + 6], ah += t[i + 7];
        fprintf(stderr,
                "ikpso coop timing: %d workgroups, per iteration (wave 0): step %.0f, argmin barrier %.0f, "
                "hand-off %.0f cycles (of which publish + draws ahead %.0f); improving exchanges %.3f (won by "
                "another chunk %.3f), key polls %.2f\n",
                s->pending_timing_n, a / it, c / it, b / it, ah / it, imp / it, rem / it, pol / it);
    }
#endif
    if (!err) {
        p.active = false;
        return IKPSO_OK;
    }
    // A group gave up waiting for its members (the GPU is shared): restore the
    // generator states and solve the whole batch on the streaming kernels.
    IKPSO_HIP(hipMemcpyAsync(s->rng, s->rng_snap, sizeof(ikpso_rng_state) * (size_t)p.args.num_swarms * s->P,
                             hipMemcpyDeviceToDevice, p.stream));
    // the cooperative workspace is idle now (the launch has completed): the
    // streaming solve runs in it, grown as needed, so no second workspace is held
    const ikpso_status st = solve_streaming(s, p.args, p.stream);
    if (st != IKPSO_OK) return st;
    IKPSO_HIP(hipStreamSynchronize(p.stream));
    p.active = false;
    ++s->fallbacks;
    g_coop_fallbacks.fetch_add(1);
    return IKPSO_OK;
}

int64_t ikpso_solver_fallbacks(const ikpso_solver* s) { return s ? s->fallbacks : 0; }

ikpso_status ikpso_solver_generator_states(ikpso_solver* s, int64_t first_swarm, int64_t count, void* dst, void* stream)
{
    if (!s || first_swarm < 0 || count < 0 || (count > 0 && !dst) || first_swarm + count > s->capacity)
        return IKPSO_ERR_INVALID_ARG;
    if (s->pending.active) {
        const ikpso_status st = ikpso_solver_sync(s);
        if (st != IKPSO_OK) return st;
    }
    if (count == 0) return IKPSO_OK;
    const hipStream_t hs = (hipStream_t)stream;
    IKPSO_HIP(hipMemcpyAsync(dst, s->rng + (size_t)first_swarm * s->P, sizeof(ikpso_rng_state) * (size_t)count * s->P,
                             hipMemcpyDefault, hs));
    IKPSO_HIP(hipStreamSynchronize(hs));
    return IKPSO_OK;
}

int64_t ikpso_coop_fallbacks(void) { return g_coop_fallbacks.load(); }

ikpso_status ikpso_solver_evaluate(ikpso_solver* s, const float* angles, const float* targets, const float* rest,
                                   int64_t n, float* out_fitness, float* out_positions, void* stream)
{
    if (!s || n < 0 || (n > 0 && !angles)) return IKPSO_ERR_INVALID_ARG;
    EvalIO io{angles, targets, rest, out_fitness, out_positions, n};
    IKPSO_HIP(launch_evaluate(s->chain, s->mode, io, (hipStream_t)stream));
    return IKPSO_OK;
}

// ikpso_solver_evaluate on the kernels that keep the node rotations: every solver evaluate serves, the
// rotation term of ikpso_solve_track_frames in the fitness.  The weights go by value (EvalFramesIO::rot_w).
ikpso_status ikpso_solver_evaluate_frames(ikpso_solver* s, const float* angles, const float* targets,
                                          const float* rest, const float* target_rot, const float* rot_weights,
                                          int64_t n, float* out_fitness, float* out_positions, float* out_rotations,
                                          float* out_rot_error, void* stream)
{
    EvalFramesIO io{};
    if (!rot_term_args(s, angles, n, true, rot_weights, target_rot, out_rot_error != nullptr, io.rot_w))
        return IKPSO_ERR_INVALID_ARG;
    io.e = EvalIO{angles, targets, rest, out_fitness, out_positions, n};
    io.target_rot = target_rot;
    io.out_rotations = out_rotations;
    io.out_rot_error = out_rot_error;
    IKPSO_HIP(launch_evaluate_frames(s->chain, s->mode, io, (hipStream_t)stream));
    return IKPSO_OK;
}

// ikpso_solver_evaluate's angle vectors on the Jacobian kernels: every solver evaluate serves, no targets,
// rest pose or weights (the Jacobian depends on none of them).
ikpso_status ikpso_solver_evaluate_jacobian(ikpso_solver* s, const float* angles, int64_t n, float* out_positions,
                                            float* out_jacobian, void* stream)
{
    if (!s || n < 0 || (n > 0 && (!angles || !out_jacobian))) return IKPSO_ERR_INVALID_ARG;
    JacobianIO io{};
    io.angles = angles;
    io.out_positions = out_positions;
    io.out_jacobian = out_jacobian;
    io.n = n;
    IKPSO_HIP(launch_evaluate_jacobian(s->chain, s->mode, io, (hipStream_t)stream));
    return IKPSO_OK;
}

// ikpso_solver_evaluate_frames' inputs on the gradient kernels: every solver evaluate serves; the fitness of
// that entry and its derivative with respect to every free angle.
ikpso_status ikpso_solver_evaluate_gradient(ikpso_solver* s, const float* angles, const float* targets,
                                            const float* rest, const float* target_rot, const float* rot_weights,
                                            int64_t n, float* out_fitness, float* out_gradient, void* stream)
{
    GradientIO io{};
    if (!rot_term_args(s, angles, n, out_gradient != nullptr, rot_weights, target_rot, false, io.rot_w))
        return IKPSO_ERR_INVALID_ARG;
    io.angles = angles;
    io.targets = targets;
    io.rest = rest;
    io.target_rot = target_rot;
    io.out_fitness = out_fitness;
    io.out_gradient = out_gradient;
    io.n = n;
    IKPSO_HIP(launch_evaluate_gradient(s->chain, s->mode, io, (hipStream_t)stream));
    return IKPSO_OK;
}

// ikpso_solver_evaluate_jacobian's angle vectors on the contacts kernels: every solver evaluate serves.  One
// word per vector and collider of the caller's descriptor; a solver whose colliders were all pruned (or that
// was given none) has nothing to decide: zeros, and the positions from the plain evaluate kernel.
ikpso_status ikpso_solver_evaluate_contacts(ikpso_solver* s, const float* angles, int64_t n, uint32_t* out_contacts,
                                            float* out_positions, void* stream)
{
    if (!s || n < 0 || (n > 0 && (!angles || (s->chain.coll_given > 0 && !out_contacts))))
        return IKPSO_ERR_INVALID_ARG;
    if (n == 0) return IKPSO_OK;
    const hipStream_t hs = (hipStream_t)stream;
    const ChainHost& ch = s->chain;
    if (ch.num_coll == 0) {
        if (ch.coll_given > 0)
            IKPSO_HIP(hipMemsetAsync(out_contacts, 0, sizeof(uint32_t) * (size_t)n * ch.coll_given, hs));
        if (out_positions) {
            EvalIO io{angles, nullptr, nullptr, nullptr, out_positions, n};
            IKPSO_HIP(launch_evaluate(ch, s->mode, io, hs));
        }
        return IKPSO_OK;
    }
    ContactsIO io{};
    io.angles = angles;
    io.out_contacts = out_contacts;
    io.out_positions = out_positions;
    io.n = n;
    io.columns = ch.coll_given;
    io.column_of = reinterpret_cast<const int32_t*>(s->aux + ch.aux.size());
    IKPSO_HIP(launch_evaluate_contacts(ch, s->mode, io, hs));
    return IKPSO_OK;
}

int ikpso_solver_dof(const ikpso_solver* s) { return s ? s->chain.dof() : 0; }
int ikpso_solver_effectors(const ikpso_solver* s) { return s ? s->chain.E : 0; }
int ikpso_solver_collider_count(const ikpso_solver* s) { return s ? s->chain.num_coll : 0; }
const char* ikpso_solver_kernel_name(const ikpso_solver* s) { return s ? s->kname[s->last].c_str() : ""; }

}  // extern "C"
