// Host side of the C ABI declared in include/gs_amd.h: context, CRS tables,
// per-shape task tables ("plans"), kernel launches.  No CPU fallback: every
// compute entry point needs a working HIP device.
#include "../../include/gs_amd.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <dlfcn.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "gs_params_bls12_381.h"
#include "gs_params_bn254.h"
#include "gs_kernels.cuh"
#include "gs_rand.cuh"
#include "gs_layout.h"

namespace gs {
GS_ZERO_ONE(Bls12_381)
GS_ZERO_ONE(Bn254)
}  // namespace gs
using namespace gs;

#define GS_VERSION "gs-amd 0.1 (gfx950)"

// ---------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};
struct ProfEntry {
  double ms = 0;
  uint64_t n = 0;
  uint64_t lanes = 0;  // lane-tasks launched
  uint64_t work = 0;   // kernel-specific work items (scalars, slots, pairs ...; = lanes when no hint was given)
  // clock stamps of the segmented launches (k_seg): sums over their waves of d s_memtime / d s_memrealtime
  double cyc = 0, rt = 0;
};

// Everything derived from one CRS on one device: immutable once built, shared (reference-counted) by every context of
// this process that installs the same CRS bytes on the same device -- Rayon-style callers keep one context per worker
// and would otherwise hold 1.8 GB of identical 16-bit window tables each.
struct CrsTables {
  int device = 0, curve = 0;
  std::vector<uint8_t> crs_bytes;
  DevBuf crs_g1;   // 6 G1 points: u0.0 u0.1 u1.0 u1.1 W1.0 W1.1
  DevBuf crs_g2;   // 6 G2 points: v0.0 v0.1 v1.0 v1.1 W2.0 W2.1
  DevBuf tab16_g1, tab16_g2;  // 16-bit window tables (k_build_tables16), what k_fix reads
  DevBuf line_tab;  // Miller line tables of the 6 CRS G2 points (k_line_tables)
  ~CrsTables() {
    hipSetDevice(device);
    for (DevBuf* b : {&crs_g1, &crs_g2, &tab16_g1, &tab16_g2, &line_tab})
      if (b->p) hipFree(b->p);
  }
};
static std::mutex g_tables_mu;
static std::vector<std::weak_ptr<CrsTables>> g_tables;

struct PlanEntry {  // an uploaded task table: device copy + the host bytes it was made from
  DevBuf dev;
  std::vector<uint8_t> host;
  uint64_t last_use = 0;
};

struct gs_ctx {
  int curve = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  bool have_crs = false;
  std::string err;
  std::shared_ptr<CrsTables> tabs;  // CRS-derived device data (shared between contexts, see CrsTables)
  // scratch
  std::map<std::string, DevBuf> scratch;
  std::map<std::string, PlanEntry> plans;  // task tables by (name, size, content hash); content compared on a hit
  uint64_t plan_clock = 0;
  std::map<std::string, std::pair<int, double>> miller_choice;  // planner decisions by (shape, N, overrides)
  // profiling
  bool prof = false;
  std::map<std::string, ProfEntry> prof_map;
  std::vector<std::string> prof_order;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  uint64_t work_hint = 0;  // consumed by the next launch() while profiling
  // Internal side streams: the fixed-base and variable-base kernels of a side, and the G1 and G2 sides of a proof,
  // are independent until their reductions; on small batches none of them fills the chip on its own.
  hipStream_t side[3] = {nullptr, nullptr, nullptr};
  hipEvent_t sev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipStream_t cur = nullptr;  // launch target override (nullptr = the context's stream)
  bool overlap = true;
  // SIMD slots of the device (CUs x 4); every heavy kernel runs one 512-VGPR wave per SIMD
  size_t simd_slots = 1024;
  // planner overrides (gs_set_option; 0 / -1 = planned per batch)
  int var_tm = 0;
  int red_k = 0;  // outputs per reduction lane (1, 2, 4); 0 = planned
  int var_ws_lanes = 0;  // Straus lanes per launch (their table workspace is 3.5 .. 28 KB each); 0 = 2^19
  int var_mo = 0, var_w = 0;  // outputs per Straus lane (1, 2, 4) and its window width (4, 5); 0 = planned
  int miller_ch = 0, miller_twin = -1;
  int coop_fe = 1;  // 0 never, 1 when one lane per final exponentiation cannot fill the chip, 2 always
  int eq_pi = -1;    // gs_verify_equation_rlc's pi term: 0 per-proof pairs, 1 folded in G2 across the batch; -1 = planned
  int locate_k = 0;  // arity of gs_verify_batch_rlc_locate's product tree (2, 4, 8); 0 = planned (8, as gt_product)
  bool line_tables = true;  // pairs whose G2 argument is a CRS element read precomputed Miller lines
  // host-pointer entry points (HostPipe below): pinned staging, a copy stream, memcpy workers, per-array events
  struct HostPipe* pipe = nullptr;  // set while a host-pointer call is enqueuing its kernels
  struct CopyPool* pool = nullptr;
  hipStream_t copy_stream = nullptr;
  void* pin = nullptr;
  size_t pin_cap = 0;
  hipEvent_t pev[16] = {nullptr};
  // mixed calls: launches are recorded per part and merged (launch_seg / replay); scratch buffers get a per-part tag;
  // the lane-shape planners see the batch size the merged launches will have
  struct Recorder* rec = nullptr;
  // 1: GLV / psi-GLS scalar multiplications (r-torsion points only, as arkworks' deserialisation guarantees); 0: every
  // variable-base scalar multiplication is a plain signed-window double-and-add lane (k_var.plain): ANY curve point,
  // like the reference's Com::scalar_mul (data_structures.rs:336-342), ~2.5x the variable-base work
  bool endo = true;
  int var_w2 = -1;  // G1 Straus lanes in the kernels built for two waves per SIMD: -1 planned, 0 never, 1 always
  int var_tab = -1;      // verifier's Gamma^T c on shared per-base window tables: -1 planned (large arities), 0, 1
  int mixed_merge = -1;  // -1 planned (merge while the parts cannot fill the chip on their own), 0 never, 1 always
  int scratch_tag = 0;
  size_t fill_n = 0;
  hipStream_t copy_stream2 = nullptr, copy_out_stream = nullptr, copy_out_stream2 = nullptr;  // two per direction
  hipEvent_t pev2[16] = {nullptr};
  hipEvent_t pev_ready = nullptr;
  // buffers a regrow or a plan eviction would have freed WHILE a mixed call records its launches (c->rec): the recorded
  // argument packs hold raw device pointers, so nothing is freed until the replay has been enqueued and drained
  std::vector<void*> deferred_free;
  unsigned long long* stamp = nullptr;  // 3 x u64 on the device: the clock stamps of the launch being profiled
  // binding key (gs_set_extraction_key), kept ONLY as its digit streams on the device: SharedDigits[4] = G1 with and
  // without the endomorphism, G2 likewise.  They are the secret: zeroed when the key goes (clear_extraction_key).
  DevBuf xkey;
  bool have_xkey = false;
  // simulation trapdoor (gs_set_simulation_key): t1, t2 as two Montgomery Fr in device memory, read by k_prep_sim alone.
  // A secret like the binding key: zeroed when the key goes (clear_simulation_key).
  DevBuf skey;
  bool have_skey = false;
  // ChaCha20 key of the device generator (gs_rand_set_key): 32 bytes in device memory, read by k_rand_fr / k_rand_rho
  // alone.  A secret like the two above, but not tied to the CRS: zeroed when the key goes (clear_rand_key).
  DevBuf rkey;
  bool have_rkey = false;
  // baby-step tables of gs_dlog_prepare, one per group ([0] G1, [1] G2): public data, not tied to the CRS
  struct DlogTab {
    DevBuf slots;  // 2^(log2_table + 1) x u64
    DevBuf aux;    // the base point (boundary bytes, padded to 256) followed by the K giant steps (internal form)
    unsigned log2_table = 0;
    bool ready = false;
  } dlog[2];
  int dlog_steps = 0;    // giant steps per launch; 0 = DLOG_STEPS_DEFAULT
  int dlog_fp_bits = 0;  // fingerprint bits compared on a lookup; 0 = all of them
};

// Every live context of the process (gs_ctx_create .. gs_ctx_destroy): page-locked caller ranges are process-wide
// (g_reg below), so releasing one has to drain the copy queues of EVERY context that may be moving it -- the shards of
// a gs_multi context are contexts of their own.
static std::mutex g_ctx_mu;
static std::vector<gs_ctx*> g_ctx_all;
// all DMA and kernels of one context done (its compute stream, side streams and the four copy streams)
static void drain_ctx(gs_ctx* c) {
  hipStreamSynchronize(c->stream);
  for (hipStream_t st : c->side)
    if (st) hipStreamSynchronize(st);
  for (hipStream_t st : {c->copy_stream, c->copy_stream2, c->copy_out_stream, c->copy_out_stream2})
    if (st) hipStreamSynchronize(st);
}

static int fail(gs_ctx* c, int code, const char* what, hipError_t e = hipSuccess) {
  if (c) {
    c->err = what;
    if (e != hipSuccess) {
      c->err += ": ";
      c->err += hipGetErrorString(e);
    }
  }
  return code;
}
#define HIPCHK(ctx, call)                                          \
  do {                                                             \
    hipError_t e_ = (call);                                        \
    if (e_ != hipSuccess) return fail(ctx, GS_ERR_DEVICE, #call, e_); \
  } while (0)

#define RC(...)                   \
  do {                            \
    int rc_ = (__VA_ARGS__);      \
    if (rc_ != GS_OK) return rc_; \
  } while (0)

static int ensure(gs_ctx* c, DevBuf& b, size_t bytes) {
  if (bytes <= b.cap && b.p) return GS_OK;
  if (b.p) {  // growing: kernels already enqueued may still read the old buffer
    if (c && c->rec) {
      // recording: nothing has been launched, a sync protects nothing -- the launches that will read the old buffer
      // are in the recorder.  Park it; mixed_dev / mixed_host release the list after the replay.
      c->deferred_free.push_back(b.p);
    } else {
      if (c) {
        hipStreamSynchronize(c->stream);
        for (hipStream_t st : c->side)
          if (st) hipStreamSynchronize(st);
      }
      hipFree(b.p);
    }
  }
  b.p = nullptr;
  b.cap = 0;
  size_t want = bytes < 256 ? 256 : bytes;
  hipError_t e = hipMalloc(&b.p, want);
  if (e != hipSuccess) return fail(c, GS_ERR_ALLOC, "hipMalloc", e);
  b.cap = want;
  return GS_OK;
}
static int scratch(gs_ctx* c, const char* name, size_t bytes, void** out) {
  char tagged[96];
  if (c->scratch_tag) {  // a part of a mixed call: its buffers are live next to the other parts'
    snprintf(tagged, sizeof tagged, "m%d:%s", c->scratch_tag, name);
    name = tagged;
  }
  DevBuf& b = c->scratch[name];
  int rc = ensure(c, b, bytes);
  *out = b.p;
  return rc;
}

// ---- external-profiler markers ("tracing") ---------------------------------------------
// roctxRangePush / Pop around the phases of prove and verify so that `rocprofv3 --marker-trace` segments a step.
// librocprofiler-sdk-roctx (or the older libroctx64) is bound at run time and only if present; without it the ranges
// are no-ops.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    const char* names[] = {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"};
    void* h = nullptr;
    for (const char* n : names)
      if ((h = dlopen(n, RTLD_NOW | RTLD_NOLOAD | RTLD_LOCAL))) break;
    if (!h && getenv("GS_ROCTX"))  // not mapped by a profiler: load it only when asked to
      for (const char* n : names)
        if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h) return;
    push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
    pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!push || !pop) push = nullptr, pop = nullptr;
  }
};
static Roctx& roctx() {
  static Roctx r;
  return r;
}
struct RangeGuard {
  bool on;
  explicit RangeGuard(const char* name) : on(roctx().push != nullptr) {
    if (on) roctx().push(name);
  }
  ~RangeGuard() {
    if (on) roctx().pop();
  }
};

// ---- host-pointer pipeline ---------------------------------------------------------------------------------------
// What a drop-in caller hands over are host slices (prove.rs:29-52, verifier.rs:18-21).  Pageable hipMemcpy on the
// compute stream cost 15 % of a 2^16 step (profiles/r2/host_path_rate.txt).  The un-suffixed entry points now
//   1. copy every input array into a grow-only PINNED staging buffer with a few memcpy worker threads (CopyPool),
//      arrays in the order the kernels need them;
//   2. enqueue the H2D of an array on a separate copy stream as soon as its staging copy is complete, with one event
//      per array;
//   3. let the engine wait for exactly the arrays the next kernels read (need(): scalars before the preparation
//      kernel, the G1 arguments before the G1 side, the G2 arguments before the G2 side / the Miller loop), so that the
//      upload of the later arrays runs under the kernels of the earlier ones;
//   4. bring the outputs back array by array (D2H into pinned memory, then the workers copy into the caller's
//      buffers while the next array is in flight).
// Equation-chunking the kernels instead would cost more than it hides: the lane shapes want whole batches (2^12
// equations run at 0.6 of the 2^16 rate).
struct CopyPool {
  struct Job {
    void* dst;
    const void* src;
    size_t n;
    std::atomic<int>* left;
  };
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Job> q;
  bool stop = false;
  explicit CopyPool(int nthreads) {
    for (int i = 0; i < nthreads; i++)
      th.emplace_back([this] {
        for (;;) {
          Job j;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [this] { return stop || !q.empty(); });
            if (q.empty()) return;
            j = q.front();
            q.pop_front();
          }
          memcpy(j.dst, j.src, j.n);
          j.left->fetch_sub(1, std::memory_order_release);
        }
      });
  }
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv.notify_all();
    for (auto& t : th) t.join();
  }
  // copy [src, src + n) to dst in pieces; *left counts the pieces still to do
  void submit(void* dst, const void* src, size_t n, std::atomic<int>* left) {
    // 2 MB pieces for large arrays; a mid-size array (the 1.5-6 MB arrays of a 2^12 batch) is cut finer so that every
    // worker gets a share of it
    size_t piece = n / (2 * th.size() + 1);
    piece = std::min(std::max(piece, (size_t)256 << 10), (size_t)2 << 20) & ~(size_t)4095;
    size_t np = (n + piece - 1) / piece;
    left->fetch_add((int)np, std::memory_order_relaxed);
    {
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < np; i++) {
        size_t o = i * piece;
        q.push_back(Job{(uint8_t*)dst + o, (const uint8_t*)src + o, std::min(piece, n - o), left});
      }
    }
    cv.notify_all();
  }
  static void wait(std::atomic<int>* left) {
    while (left->load(std::memory_order_acquire) > 0) std::this_thread::yield();
  }
};

static std::mutex g_reg_mu;
static std::map<const uint8_t*, size_t> g_reg;  // gs_host_register: start -> bytes
struct HostPipe {
  struct Arr {
    const void* hin = nullptr;
    void* hout = nullptr;
    void* d = nullptr;
    size_t bytes = 0, off = 0;
    std::atomic<int> left{0};
    bool enq = false;
    bool direct = false;  // the caller's array is page-locked already: DMA to / from it, no staging copy
  };
  // Page-locked caller memory is what was registered through gs_host_register -- the library's own list, nothing else.
  // (The first version asked the runtime, hipPointerGetAttributes on both ends of the array.  That also reports ranges
  // the runtime itself has pinned behind the caller's back -- the source of an earlier pageable hipMemcpy, kept in its
  // pin cache, possibly mapped READ-ONLY, possibly belonging to a buffer that has been freed since and whose addresses a
  // new array now occupies.  A D2H straight into such a range ended in "write access to a read-only page" on the GPU.)
  static bool host_pinned(const void* p, size_t bytes);
  gs_ctx* c;
  Arr arr[16];
  hipEvent_t ev1[16] = {nullptr}, ev2[16] = {nullptr};
  int out_order[16], n_out = 0;  // output arrays in the order their D2H went out (= the order they arrive)
  int n = 0;
  bool trace = false;
  bool begun = false, finished = false;  // begin() has enqueued work on the copy streams / finish() has waited for all of it
  int split = 2;  // DMA transfers per array and direction (two copy streams: two SDMA engines)
  std::chrono::steady_clock::time_point t0;
  explicit HostPipe(gs_ctx* ctx) : c(ctx) {}
  ~HostPipe() {
    for (int i = 0; i < n; i++) CopyPool::wait(&arr[i].left);  // no worker may still touch the caller's memory
    // A call that failed between begin() and the end of finish() returns with H2D / D2H still queued against the caller's
    // (possibly page-locked) arrays and against stage.* buffers the next call will overwrite: nothing may be in flight
    // when the caller gets the error back and unwinds (unregisters, frees).
    if (begun && !finished) drain_ctx(c);
    for (int i = 0; i < 16; i++)
      for (hipEvent_t ev : {ev1[i], ev2[i]})
        if (ev) hipEventDestroy(ev);
    if (c->pipe == this) c->pipe = nullptr;
  }
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
  // declare array `i` (slots are fixed per entry point: the need() masks name them); null / empty arrays stay absent
  int in(int i, const void* h, size_t bytes) {
    if (h && bytes) arr[i].hin = h, arr[i].bytes = bytes;
    n = std::max(n, i + 1);
    return GS_OK;
  }
  int out(int i, void* h, size_t bytes) {
    if (h && bytes) arr[i].hout = h, arr[i].bytes = bytes;
    n = std::max(n, i + 1);
    return GS_OK;
  }
  void* dev(int i) const { return arr[i].d; }
  // bytes of pinned staging this call needs (every declared array, 256-byte aligned)
  size_t layout() {
    size_t total = 0;
    for (int i = 0; i < n; i++) {
      if (!arr[i].bytes) continue;
      arr[i].direct = host_pinned(arr[i].hin ? arr[i].hin : arr[i].hout, arr[i].bytes);
      if (arr[i].direct) continue;
      arr[i].off = total;
      total += (arr[i].bytes + 255) & ~(size_t)255;
    }
    return total;
  }
  // the context's grow-only pinned buffer holds at least `bytes` (never call between begin() and finish() of a pipe
  // that uses it: growing moves it)
  static int pin_reserve(gs_ctx* c, size_t bytes) {
    if (bytes <= c->pin_cap) return GS_OK;
    if (c->pin) hipHostFree(c->pin);
    c->pin = nullptr;
    c->pin_cap = 0;
    hipError_t e = hipHostMalloc(&c->pin, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, GS_ERR_ALLOC, "hipHostMalloc (pinned staging)", e);
    c->pin_cap = bytes;
    return GS_OK;
  }
  // device slots, workers; then the staging copies start, inputs in the order `order` lists them.  `base`: where this
  // pipe's region of the pinned buffer begins (several pipes of one mixed call share the buffer)
  int begin(const int* order, int norder, size_t base = 0, bool reserve = true) {
    begun = true;
    t0 = std::chrono::steady_clock::now();
    trace = getenv("GS_PIPE_TRACE") != nullptr;
    if (const char* e = getenv("GS_COPY_SPLIT")) split = std::max(1, std::min(2, atoi(e)));
    // The copy streams are created at HIGH priority, which is not about urgency: the runtime multiplexes the streams
    // of one priority level over a few hardware queues (4 by default), and a copy stream that lands on the compute
    // stream's queue is serialized with the kernels there -- the first kernel then starts only after EVERY upload
    // enqueued before it, and uploads enqueued behind a long kernel wait for that kernel
    // (profiles/r3/host_pipe_timeline.txt).  Another priority level is another set of queues.
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    for (hipStream_t* st : {&c->copy_stream, &c->copy_stream2, &c->copy_out_stream, &c->copy_out_stream2})
      if (!*st && hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio_greatest) != hipSuccess) {
        (void)hipGetLastError();  // no priority levels here: an ordinary stream (correct, possibly serialized as above)
        *st = nullptr;
        HIPCHK(c, hipStreamCreateWithFlags(st, hipStreamNonBlocking));
      }
    if (!c->pev_ready) HIPCHK(c, hipEventCreateWithFlags(&c->pev_ready, hipEventDisableTiming));
    if (!c->pool) {
      int nt = 4;
      if (const char* e = getenv("GS_COPY_THREADS")) nt = std::max(1, std::min(32, atoi(e)));
      c->pool = new CopyPool(nt);
    }
    const size_t total = layout();
    if (reserve) RC(pin_reserve(c, base + total));
    for (int i = 0; i < n; i++) {
      if (!arr[i].bytes) continue;
      char name[32];
      snprintf(name, sizeof name, "stage.%d", i);
      RC(scratch(c, name, arr[i].bytes, &arr[i].d));
      arr[i].off += base;
      // events are per (pipe, array): a mixed call has several pipes in flight
      for (hipEvent_t* ev : {&ev1[i], &ev2[i]}) HIPCHK(c, hipEventCreateWithFlags(ev, hipEventDisableTiming));
    }
    for (int k = 0; k < norder; k++) {
      Arr& a = arr[order[k]];
      if (a.hin && !a.direct) c->pool->submit((uint8_t*)c->pin + a.off, a.hin, a.bytes, &a.left);
    }
    for (int k = 0; k < norder; k++) {  // page-locked inputs need no staging: their uploads go out at once
      Arr& a = arr[order[k]];
      if (!a.hin || !a.direct || a.enq) continue;
      RC(xfer(a.d, a.hin, a.bytes, hipMemcpyHostToDevice, c->copy_stream, c->copy_stream2, ev1[order[k]], ev2[order[k]]));
      a.enq = true;
    }
    c->pipe = this;
    if (trace) fprintf(stderr, "[pipe] %7.2f ms begin done (%zu bytes of staging)\n", ms(), total);
    return GS_OK;
  }
  // (begun is set at the top of begin(): a begin() that fails half way has already queued copies)
  // one array across PCIe, in `split` pieces on as many copy streams; ev is recorded (on s0) behind all of them
  int xfer(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s0, hipStream_t s1, hipEvent_t ev,
           hipEvent_t ev_b) {
    if (split < 2 || bytes < ((size_t)4 << 20)) {
      HIPCHK(c, hipMemcpyAsync(dst, src, bytes, kind, s0));
    } else {
      size_t h = (bytes / 2 + 255) & ~(size_t)255;
      HIPCHK(c, hipMemcpyAsync(dst, src, h, kind, s0));
      HIPCHK(c, hipMemcpyAsync((uint8_t*)dst + h, (const uint8_t*)src + h, bytes - h, kind, s1));
      HIPCHK(c, hipEventRecord(ev_b, s1));
      HIPCHK(c, hipStreamWaitEvent(s0, ev_b, 0));
    }
    HIPCHK(c, hipEventRecord(ev, s0));
    return GS_OK;
  }
  // the kernels about to be enqueued read the input arrays in `mask`: their uploads go out (if they have not yet)
  // and the target stream waits for them
  int need(unsigned mask) {
    hipStream_t tgt = c->cur ? c->cur : c->stream;
    for (int i = 0; i < n; i++) {
      Arr& a = arr[i];
      if (!((mask >> i) & 1) || !a.hin) continue;
      if (!a.enq) {
        double w0 = trace ? ms() : 0;
        CopyPool::wait(&a.left);
        double w1 = trace ? ms() : 0;
        RC(xfer(a.d, a.direct ? a.hin : (uint8_t*)c->pin + a.off, a.bytes, hipMemcpyHostToDevice, c->copy_stream, c->copy_stream2, ev1[i],
                ev2[i]));
        a.enq = true;
        if (trace)
          fprintf(stderr, "[pipe] %7.2f ms H2D of array %d enqueued (%.1f MB, waited %.2f ms for its staging, %.2f ms in the enqueue)\n",
                  ms(), i, a.bytes / 1e6, w1 - w0, ms() - w1);
      }
      HIPCHK(c, hipStreamWaitEvent(tgt, ev1[i], 0));
    }
    return GS_OK;
  }
  // the output arrays in `mask` are complete once the work enqueued so far on the current stream is done: their D2H
  // starts behind it on the copy-out streams, under whatever kernels follow
  int out_ready(unsigned mask) {
    if (c->rec) return GS_OK;  // launches are only being recorded: nothing has been computed yet
    hipStream_t src = c->cur ? c->cur : c->stream;
    bool first = true;
    for (int i = 0; i < n; i++) {
      Arr& a = arr[i];
      if (!((mask >> i) & 1) || !a.hout || a.enq) continue;
      if (first) {
        HIPCHK(c, hipEventRecord(c->pev_ready, src));
        HIPCHK(c, hipStreamWaitEvent(c->copy_out_stream, c->pev_ready, 0));
        HIPCHK(c, hipStreamWaitEvent(c->copy_out_stream2, c->pev_ready, 0));
        first = false;
      }
      RC(xfer(a.direct ? a.hout : (uint8_t*)c->pin + a.off, a.d, a.bytes, hipMemcpyDeviceToHost, c->copy_out_stream, c->copy_out_stream2,
              ev1[i], ev2[i]));
      a.enq = true;
      out_order[n_out++] = i;
      if (trace) fprintf(stderr, "[pipe] %7.2f ms D2H of array %d enqueued (%.1f MB)\n", ms(), i, a.bytes / 1e6);
    }
    return GS_OK;
  }
  // outputs: D2H per array behind the kernels, each copied on to the caller's buffer while the next one is in flight
  int finish() {
    c->pipe = nullptr;
    if (trace) fprintf(stderr, "[pipe] %7.2f ms kernels enqueued\n", ms());
    hipStream_t keep = c->cur;
    c->cur = nullptr;
    int rc = out_ready(0xFFFFu);  // whatever has not gone out yet, behind the last kernel
    c->cur = keep;
    RC(rc);
    for (int k = 0; k < n_out; k++) {  // in arrival order: an early array is on its way to the caller while later ones fly
      const int i = out_order[k];
      Arr& a = arr[i];
      HIPCHK(c, hipEventSynchronize(ev1[i]));
      if (trace) fprintf(stderr, "[pipe] %7.2f ms array %d arrived\n", ms(), i);
      if (!a.direct) c->pool->submit(a.hout, (uint8_t*)c->pin + a.off, a.bytes, &a.left);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++) CopyPool::wait(&arr[i].left);
    // (every D2H was waited for through its event above; the H2D queues were waited for by the kernels that the
    // stream sync has just seen finish)
    finished = true;
    if (trace) fprintf(stderr, "[pipe] %7.2f ms done\n", ms());
    return GS_OK;
  }
};
bool HostPipe::host_pinned(const void* p, size_t bytes) {
  static const bool off = getenv("GS_PIPE_NO_DIRECT") != nullptr;
  if (off || !p || !bytes) return false;
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto it = g_reg.upper_bound((const uint8_t*)p);
  if (it == g_reg.begin()) return false;
  --it;  // the last registration that starts at or before p
  return (const uint8_t*)p + bytes <= it->first + it->second;
}
static inline int need(gs_ctx* c, unsigned mask) { return c->pipe ? c->pipe->need(mask) : GS_OK; }
static inline int out_ready(gs_ctx* c, unsigned mask) { return c->pipe ? c->pipe->out_ready(mask) : GS_OK; }
// array slots of the host-pointer entry points
enum { PI_X = 0, PI_Y, PI_A, PI_B, PI_G, PI_R, PI_S, PI_T, PO_XC, PO_YC, PO_PI, PO_TH };           // prove
enum { VI_A = 0, VI_B, VI_G, VI_TG, VI_XC, VI_YC, VI_PI, VI_TH, VO_OK };                            // verify
enum { RI_A = 0, RI_B, RI_G, RI_R, RI_S, RI_T, RI_XC, RI_YC, RI_PI, RI_TH, RO_XC, RO_YC, RO_PI, RO_TH };  // rerandomize
enum { EI_X = 0, EI_Y, EI_A, EI_B, EI_G, EI_TG, EO_T, EO_OK };                                      // evaluate / check witness
enum { SI_A = 0, SI_B, SI_G, SI_TG, SI_R, SI_S, SI_T, SO_XC, SO_YC, SO_PI, SO_TH };                 // simulate
#define BIT(i) (1u << (i))

// the batch size the lane-shape planners should fill the chip for: the part's own, or (mixed calls, whose parts'
// launches are merged) the whole call's
static inline size_t fillN(const gs_ctx* c, size_t N) { return c->fill_n > N ? c->fill_n : N; }

// ---- Miller-lane planning --------------------------------------------------------------------------
// A Miller lane carries up to MILLER_CH (P, Q) pairs (twin: (Q, P0, P1) triples with two accumulators) and squares its
// own accumulator every iteration, so longer lanes do less total work but a small batch needs many short ones to fill
// the chip.  Pairs whose G2 argument is a CRS element read precomputed lines and are cheaper.  Cost model (checked
// against measurements at 2^12..2^16): rounds of waves over the SIMD slots x the longest lane, in
// Fq multiplications (profiles/r1/fq_mul_counts.json).  Lanes are task-major (a wave = 64 equations of ONE task).
struct MCost {
  double base, var, fix;
};
// whether the planner may pick the lane-pair form of the twin loop on its own (measured per round: DESIGN.md section 4.2)
#ifndef GS_PLAN_PAIR
#define GS_PLAN_PAIR 1
#endif
// (profiles/r5/fq_mul_counts.json: miller*_per_lane, _per_pair / _per_triple, _per_fixed_pair / _per_fixed_triple --
// the counts with real-form lines: stepped lines of the twin forms and every tabulated line go through the 72 L^2
// sparse product; -DGS_LINES_GENERAL has the round-3 counts of the general product)
static inline MCost mcost(int curve, bool twin) {
#if defined(GS_LINES_GENERAL)
  if (curve == 0) return twin ? MCost{4536.0, 7764.0, 6256.0} : MCost{2268.0, 4636.0, 3128.0};
  return twin ? MCost{4680.0, 10519.0, 8096.0} : MCost{2340.0, 6471.0, 4048.0};
#else
  if (curve == 0) return twin ? MCost{4536.0, 7356.0, 5304.0} : MCost{2268.0, 4636.0, 2652.0};
  return twin ? MCost{4680.0, 9991.0, 6864.0} : MCost{2340.0, 6471.0, 3432.0};
#endif
}
static inline bool pair_fixed(bool lt, const PairRef& r) { return lt && r.q_arr == 2; }  // Q array 2 = CRS (v, W2)
// Split one cell's pairs into the fewest tasks whose lane cost stays within `budget`: costly pairs first, each to the
// lightest task that still has room (LPT).
static void chunk_tasks(std::vector<MillerTask>& mt, const std::vector<PairRef>& pr, double budget, int b, bool single,
                        const MCost& mc, bool lt) {
  size_t P = pr.size();
  if (P == 0) return;
  std::vector<size_t> order;
  double total = 0;
  for (size_t i = 0; i < P; i++)
    if (!pair_fixed(lt, pr[i])) order.push_back(i);
  for (size_t i = 0; i < P; i++)
    if (pair_fixed(lt, pr[i])) order.push_back(i);
  for (size_t i = 0; i < P; i++) total += pair_fixed(lt, pr[i]) ? mc.fix : mc.var;
  // no fewer tasks than the capacity or the budget allow (large arities have hundreds of pairs per cell: start at the
  // bound instead of walking up to it, and place with a heap: O(P log P) per attempt)
  size_t nt0 = (P + MILLER_CH - 1) / MILLER_CH;
  if (budget > 0) nt0 = std::max(nt0, (size_t)(total / budget));
  nt0 = std::min(std::max(nt0, (size_t)1), P);
  for (size_t nt = nt0; nt <= P; nt++) {
    std::vector<double> load(nt, 0.0);
    std::vector<std::vector<size_t>> members(nt);
    typedef std::pair<double, size_t> Slot;  // (load, task): lightest task that still has room first
    std::priority_queue<Slot, std::vector<Slot>, std::greater<Slot>> heap;
    for (size_t t = 0; t < nt; t++) heap.push(Slot(0.0, t));
    for (size_t idx : order) {
      Slot sl = heap.top();
      heap.pop();
      size_t best = sl.second;
      members[best].push_back(idx);
      load[best] += pair_fixed(lt, pr[idx]) ? mc.fix : mc.var;
      if (members[best].size() < (size_t)MILLER_CH) heap.push(Slot(load[best], best));
    }
    double mx = 0;
    for (double l : load) mx = l > mx ? l : mx;
    if (mx > budget && nt < P) continue;
    for (size_t t = 0; t < nt; t++) {
      MillerTask mtk;
      memset(&mtk, 0, sizeof mtk);
      mtk.b = (uint8_t)b;
      mtk.single = single ? 1 : 0;
      mtk.np = (uint8_t)members[t].size();
      for (int q = 0; q < mtk.np; q++) mtk.pr[q] = pr[members[t][q]];
      mt.push_back(mtk);
    }
    return;
  }
}
// serial cost (in units of `unit`) of reducing `n` partial results: runs of 8 folded in parallel while more than 16
// are left (k_cell_fold / k_slot_fold), the rest by the consuming lane
static double fold_cost(double n, double unit) {
  double c = 0;
  while (n > 16.0) {
    c += 8.0 * unit;
    n = (double)(size_t)((n + 7.0) / 8.0);
  }
  return c + n * unit;
}
// `pair`: the twin task list run by k_miller_pair -- two lanes of half the length per (equation, task)
// A pair of lanes (k_miller_pair) is one task inside ONE wave: what the wave executes per loop digit is a squaring, one
// twist-point step per ROUND of two stepping triples (the lanes of a pair step one each; an odd triple is a round of its
// own) and one line product per triple.
static inline double pair_lane_cost(const gs_ctx* c, const MillerTask& t) {
  const MCost mc = mcost(c->curve, true);
  int nv = 0, nf = 0;
  for (int q = 0; q < t.np; q++) (pair_fixed(c->line_tables, t.pr[q]) ? nf : nv)++;
  return mc.base / 2 + ((nv + 1) / 2) * (mc.var - mc.fix) + (nv + nf) * mc.fix / 2;
}
static double miller_cost(const gs_ctx* c, size_t N, const std::vector<MillerTask>& mt, bool twin, bool pair = false) {
  MCost mc = mcost(c->curve, twin);
  // Lanes are task-major: a wave is 64 equations of ONE task and lasts as long as that task's lane.  A launch lasts
  // as long as its longest lane, or -- once it is several rounds of waves -- as long as all lanes together take on the
  // SIMD slots (waves of short tasks do not wait for those of long ones).
  double longest = 0, all = 0;
  // waves per task (below 64 equations a wave holds several tasks: a fraction of a wave each)
  const size_t NL = pair ? 2 * N : N;  // lanes per task
  const double wpt = NL >= 64 ? (double)(size_t)((NL + 63) / 64) : (double)NL / 64.0;
  for (const MillerTask& t : mt) {
    double l = mc.base;
    for (int q = 0; q < t.np; q++) l += pair_fixed(c->line_tables, t.pr[q]) ? mc.fix : mc.var;
    if (pair) l = pair_lane_cost(c, t);
    longest = l > longest ? l : longest;
    all += l * wpt;
  }
  double rounds = (double)mt.size() * wpt / (double)c->simd_slots;
  double fill = all / (double)c->simd_slots;
  if (rounds > 1.0 && rounds < 4.0) fill *= (double)(size_t)(rounds + 0.999) / rounds;  // whole rounds while few
  double lane = rounds <= 1.0 ? longest : (fill > longest ? fill : longest);
  // + the lanes that multiply a cell's partials together (54 Fq multiplications each): k_final's own serial product
  // up to 16 of them, above that K-ary tree levels of 8 (k_cell_fold; large arities)
  double per_cell = (double)mt.size() * (twin ? 2.0 : 1.0) / 4.0;
  return lane + fold_cost(per_cell, 54.0);
}
// lane-cost budgets worth trying: a variable + f fixed pairs
static std::vector<double> miller_budgets(const gs_ctx* c, bool twin) {
  const MCost mc = mcost(c->curve, twin);
  std::vector<double> out;
  for (int a = 1; a <= MILLER_CH; a++)
    for (int f = 0; f <= 2 && a + f <= MILLER_CH; f++) {
      if (c->miller_ch > 0 && a + f != c->miller_ch) continue;
      out.push_back(a * mc.var + f * mc.fix);
    }
  return out;
}
// single-accumulator task list over the pairs `pr` of an equation: the budget of least planned cost
static std::vector<MillerTask> plan_miller_single(const gs_ctx* c, size_t N, const std::vector<PairRef>& pr) {
  std::vector<MillerTask> mt;
  double best = -1;
  for (double cand : miller_budgets(c, false)) {
    std::vector<MillerTask> tmp;
    chunk_tasks(tmp, pr, cand, 0, true, mcost(c->curve, false), c->line_tables);
    double cost = miller_cost(c, N, tmp, false);
    if (best < 0 || cost < best) {
      best = cost;
      mt = tmp;
    }
  }
  return mt;
}
// work of a Miller launch: (P, Q) pairs (twin: (Q, P0, P1) triples) per equation, a table-reading pair counted at its
// cost ratio
static void miller_work_hint(gs_ctx* c, size_t N, const std::vector<MillerTask>& mt, bool twin) {
  const MCost mc = mcost(c->curve, twin);
  double pairs = 0;
  for (const MillerTask& t : mt)
    for (int q = 0; q < t.np; q++) pairs += pair_fixed(c->line_tables, t.pr[q]) ? mc.fix / mc.var : 1.0;
  c->work_hint = (uint64_t)((double)N * pairs);
}

// k_var_multi lanes per launch: their Straus tables (affine table + the Jacobian staging of its build) live in a
// per-context workspace of 9 .. 70 KB per lane (G2, 8 terms, 5-bit windows: 28 + 42 KB).  Two rounds of resident waves
// (simd_slots x 64 lanes each) keep the launch overhead below 1 % and bound the workspace at 9.2 GB for the largest
// lane whatever the batch.
static inline size_t var_ws_default(const gs_ctx* c) { return 2 * c->simd_slots * 64; }
// Straus lanes per launch.  Two rounds of resident waves is what a 2^16 batch needs; a larger batch used to run as several
// launches over that workspace, and every launch boundary idles the SIMDs whose last wave finished early (2^17 / 2^18 on
// one GPU ran 5 % below the 2^16 rate: profiles/r3/bench_log2n17/18.json).  This GPU has 288 GB: when a quarter of
// the free device memory (at most 32 GB) holds the workspace of more lanes, the launch takes them -- whole rounds of
// waves, so that a remaining chunk is never a sliver.
static size_t var_ws_auto(const gs_ctx* c, size_t tot, size_t bytes_per_lane) {
  const size_t round = c->simd_slots * 64, base = var_ws_default(c);
  if (tot <= base) return tot;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    return base;
  }
  size_t budget = std::min(free_b / 4, (size_t)32 << 30);
  size_t lanes = budget / std::max(bytes_per_lane, (size_t)1) / round * round;
  return std::min(tot, std::max(lanes, base));
}
// launch wrapper with optional HIP-event timing (used by bench.py's roofline leg)
template <class K, class... Args>
static int launch(gs_ctx* c, const char* name, K kern, size_t total, int block, Args... args) {
  if (c->rec) return fail(c, GS_ERR_ARG, "internal: this kernel cannot be part of a merged launch");
  if (total == 0) return GS_OK;
  unsigned grid = (unsigned)((total + block - 1) / block);
  hipStream_t st = c->cur ? c->cur : c->stream;
  if (c->prof) hipEventRecord(c->ev0, st);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, st, args...);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, GS_ERR_DEVICE, name, e);
  if (c->prof) {
    hipEventRecord(c->ev1, st);
    hipEventSynchronize(c->ev1);
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    if (!c->prof_map.count(name)) c->prof_order.push_back(name);
    ProfEntry& p = c->prof_map[name];
    p.ms += ms;
    p.n += 1;
    p.lanes += total;
    p.work += c->work_hint ? c->work_hint : total;
  }
  c->work_hint = 0;
  return GS_OK;
}

// ---- segmented launches (csrc/gs_kernels.cuh: k_seg) ----------------------------------------------------------------
// launch_seg<Body>(c, name, lanes, block, args...) runs a kernel BODY over one segment -- or, while a mixed call is
// recording (c->rec), only notes the launch.  replay() then walks the parts' launch lists in step and merges the launches
// that run the same body (same instantiation, same block size) into one k_seg launch with a segment per part.
struct LaunchRec {
  std::string name;
  const void* kern = nullptr;  // address of the k_seg instantiation: the identity of the body
  size_t total = 0;
  int block = 64;
  uint64_t work = 0;
  std::vector<uint8_t> pack;   // the bytes of this launch's Pack<args...>
  int (*go)(gs_ctx*, const LaunchRec* const*, int) = nullptr;
};
struct Recorder {
  std::vector<std::vector<LaunchRec>> parts;
  int cur = 0;
};
template <class Body, class... A> static int go_seg(gs_ctx* c, const LaunchRec* const* r, int nr) {
  Segs<A...> S;
  memset((void*)&S, 0, sizeof S);
  S.n = nr;
  size_t lanes = 0, tot = 0;
  uint64_t work = 0;
  const int block = r[0]->block;
  for (int i = 0; i < nr; i++) {
    S.lo[i] = lanes;
    memcpy((void*)&S.a[i], r[i]->pack.data(), sizeof(Pack<A...>));
    lanes += (r[i]->total + block - 1) / block * block;
    tot += r[i]->total;
    work += r[i]->work ? r[i]->work : r[i]->total;
  }
  if (lanes == 0) return GS_OK;
  hipStream_t st = c->cur ? c->cur : c->stream;
  if (c->prof) {
    if (!c->stamp && hipMalloc((void**)&c->stamp, 3 * sizeof(unsigned long long)) != hipSuccess) c->stamp = nullptr;
    if (c->stamp) hipMemsetAsync(c->stamp, 0, 3 * sizeof(unsigned long long), st);
    S.stamp = c->stamp;
    hipEventRecord(c->ev0, st);
  }
  hipLaunchKernelGGL((k_seg<Body, A...>), dim3((unsigned)(lanes / block)), dim3(block), 0, st, S);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, GS_ERR_DEVICE, r[0]->name.c_str(), e);
  if (c->prof) {
    hipEventRecord(c->ev1, st);
    hipEventSynchronize(c->ev1);
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    const std::string& name = r[0]->name;
    if (!c->prof_map.count(name)) c->prof_order.push_back(name);
    ProfEntry& p = c->prof_map[name];
    p.ms += ms;
    p.n += 1;
    p.lanes += tot;
    p.work += work;
    if (c->stamp) {
      unsigned long long h[3] = {0, 0, 0};
      if (hipMemcpy(h, c->stamp, sizeof h, hipMemcpyDeviceToHost) == hipSuccess) p.cyc += (double)h[0], p.rt += (double)h[1];
    }
  }
  return GS_OK;
}
// The record of a launch: what launch_seg_typed launches or notes, and what seg_pair merges
template <class Body, class... A, class... U>
static LaunchRec seg_rec_typed(gs_ctx* c, const char* name, void (*)(size_t, A...), size_t total, int block, U&&... u) {
  static_assert(sizeof...(A) == sizeof...(U), "argument count of the kernel body");
  static_assert(sizeof(Segs<A...>) <= 3800, "the segment table travels as a kernel argument");
  LaunchRec r;
  r.name = name;
  r.kern = (const void*)&k_seg<Body, A...>;
  r.total = total;
  r.block = block;
  r.work = c->work_hint;
  c->work_hint = 0;
  Pack<A...> pk{{static_cast<A>(u)}...};
  r.pack.assign((const uint8_t*)&pk, (const uint8_t*)&pk + sizeof pk);
  r.go = &go_seg<Body, A...>;
  return r;
}
template <class Body, class... A, class... U>
static int launch_seg_typed(gs_ctx* c, const char* name, void (*sig)(size_t, A...), size_t total, int block, U&&... u) {
  LaunchRec r = seg_rec_typed<Body>(c, name, sig, total, block, std::forward<U>(u)...);
  if (c->rec) {
    if (total) c->rec->parts[c->rec->cur].push_back(std::move(r));
    return GS_OK;
  }
  if (total == 0) return GS_OK;
  const LaunchRec* rp = &r;
  return r.go(c, &rp, 1);
}
template <class Body, class... U> static LaunchRec seg_rec(gs_ctx* c, const char* name, size_t total, int block, U&&... u) {
  typedef decltype(&Body::run) Sig;
  return seg_rec_typed<Body>(c, name, (Sig) nullptr, total, block, std::forward<U>(u)...);
}
// Two independent launches of ONE body as the two segments of one launch (a's lanes first); under the kernel
// profile they go out one after the other so that each keeps its own name, time and work.
static int seg_pair(gs_ctx* c, const LaunchRec& a, const LaunchRec& b) {
  if (c->rec) return fail(c, GS_ERR_ARG, "internal: this kernel cannot be part of a merged launch");
  const LaunchRec* both[2] = {&a, &b};
  if (c->prof || a.total == 0 || b.total == 0) {
    for (const LaunchRec* r : both)
      if (r->total) RC(r->go(c, &r, 1));
    return GS_OK;
  }
  return a.go(c, both, 2);
}
template <class Body, class... U> static int launch_seg(gs_ctx* c, const char* name, size_t total, int block, U&&... u) {
  typedef decltype(&Body::run) Sig;  // void (*)(size_t g, args...): the body's own parameter types
  return launch_seg_typed<Body>(c, name, (Sig) nullptr, total, block, std::forward<U>(u)...);
}
// Launch what the parts of a mixed call recorded.  Each part's list is in dependency order (it is what the part would
// have enqueued on the stream); launches of different parts are independent.  Lock-step merge: the parts whose NEXT
// launch runs the same body (same instantiation, same block size) form a group that goes out as one segmented launch.
// When the heads differ (one part has a kernel the others lack, or another variant of it), a group is taken that no
// other part could still join later -- its body does not occur further down any non-member's list -- so that the parts
// fall back into step right after it; only if every head is awaited elsewhere does the first unfinished part lead.
static int replay(gs_ctx* c, Recorder& R) {
  const size_t np = R.parts.size();
  std::vector<size_t> cur(np, 0);
  auto head = [&](size_t p) -> const LaunchRec* { return cur[p] < R.parts[p].size() ? &R.parts[p][cur[p]] : nullptr; };
  auto same = [](const LaunchRec* a, const LaunchRec* b) { return a->kern == b->kern && a->block == b->block; };
  for (;;) {
    size_t lead = np;
    for (size_t p = 0; p < np && lead == np; p++) {
      const LaunchRec* h = head(p);
      if (!h) continue;
      bool awaited = false;  // does a part that is NOT at this body now still have it ahead?
      for (size_t q = 0; q < np && !awaited; q++) {
        const LaunchRec* hq = head(q);
        if (q == p || !hq || same(hq, h)) continue;
        for (size_t k = cur[q] + 1; k < R.parts[q].size() && !awaited; k++) awaited = same(&R.parts[q][k], h);
      }
      if (!awaited) lead = p;
    }
    if (lead == np)
      for (size_t p = 0; p < np && lead == np; p++)
        if (head(p)) lead = p;
    if (lead == np) return GS_OK;
    const LaunchRec* L = head(lead);
    const LaunchRec* grp[MAX_SEG];
    int ng = 0;
    for (size_t p = 0; p < np && ng < MAX_SEG; p++) {
      const LaunchRec* h = head(p);
      if (h && same(h, L)) {
        grp[ng++] = h;
        cur[p]++;
      }
    }
    RC(L->go(c, grp, ng));
  }
}

// ---------------------------------------------------------------------------
// shape helpers
// ---------------------------------------------------------------------------
// scalar preparation goes one-lane-per-output once an equation carries this many Gamma entries
static inline bool wide_prep(int m, int n) { return (long)m * n >= 1024; }
namespace lay = gs_layout;  // the sizes of a batch's arrays (gs_layout.h)
using lay::x_is_group;
using lay::y_is_group;

template <class C> struct Sz {
  // BOUNDARY sizes (include/gs_amd.h), not the internal radix-2^28 structs
  static constexpr size_t FQ = 4 * C::N, FR = sizeof(Fr<C>), G1 = 2 * FQ, G2 = 4 * FQ, GT = 12 * FQ,
                          COM1 = 2 * G1, COM2 = 2 * G2, CRS = 2 * COM1 + 2 * COM2 + G1 + G2 + GT;
};

// table ids inside tab16_g1/tab16_g2 (and the first-level tab_g1/tab_g2): 0 u0.0, 1 u0.1, 2 u1.0, 3 u1.1, 4 W.1 ; W.0 aliases u1.0
static inline uint8_t tb_u(int k, int c) { return (uint8_t)(2 * k + c); }
static inline uint8_t tb_w(int c) { return c ? 4 : 2; }

// Task tables are immutable once uploaded: they are cached per (name, size, content hash) so that a later batch never
// overwrites a table an in-flight kernel reads.  The host bytes are kept and compared on a hit (a hash collision gets
// its own entry instead of silently reusing the wrong plan); the cache is capped: past GS_PLAN_CAP entries the least
// recently used ones are freed after a stream sync (shapes seen long ago by a long-lived context).
constexpr size_t GS_PLAN_CAP = 256;
static int plan_evict(gs_ctx* c) {
  if (c->plans.size() <= GS_PLAN_CAP) return GS_OK;
  if (c->rec) return GS_OK;  // recorded launches hold pointers into the cached tables: evict on a later call
  hipStreamSynchronize(c->stream);
  for (hipStream_t st : c->side)
    if (st) hipStreamSynchronize(st);
  while (c->plans.size() > GS_PLAN_CAP / 2) {
    auto victim = c->plans.begin();
    for (auto it = c->plans.begin(); it != c->plans.end(); ++it)
      if (it->second.last_use < victim->second.last_use) victim = it;
    if (victim->second.dev.p) hipFree(victim->second.dev.p);
    c->plans.erase(victim);
  }
  return GS_OK;
}
template <class T> static int upload(gs_ctx* c, const char* name, const std::vector<T>& v, const T** out) {
  uint64_t h = 1469598103934665603ull;
  const uint8_t* b = (const uint8_t*)v.data();
  const size_t nb = v.size() * sizeof(T);
  {  // 8 bytes per step (large-arity task tables are megabytes; the content is compared on a hit anyway)
    size_t i = 0;
    for (; i + 8 <= nb; i += 8) {
      uint64_t w;
      memcpy(&w, b + i, 8);
      h = (h ^ w) * 1099511628211ull;
      h ^= h >> 29;
    }
    for (; i < nb; i++) h = (h ^ b[i]) * 1099511628211ull;
  }
  if (getenv("GS_PLAN_TRACE")) fprintf(stderr, "[plan] table %s %zu %016llx\n", name, v.size(), (unsigned long long)h);
  for (int salt = 0;; salt++) {
    char key[176];
    snprintf(key, sizeof key, "plan%s.%zu.%016llx.%d", name, v.size(), (unsigned long long)h, salt);
    auto it = c->plans.find(key);
    if (it != c->plans.end()) {
      PlanEntry& e = it->second;
      if (e.host.size() != nb || (nb && memcmp(e.host.data(), b, nb) != 0)) continue;  // collision: next salt
      if (!e.dev.p) {  // (cannot happen since entries are inserted after their upload; never hand out a null table)
        c->plans.erase(it);
        continue;
      }
      e.last_use = ++c->plan_clock;
      *out = (const T*)e.dev.p;
      return GS_OK;
    }
    RC(plan_evict(c));
    // the entry goes into the cache only once its device copy exists: a failed allocation or copy must not leave a
    // key behind that a later call (same shape, e.g. a retry with a smaller batch) would hit with a null table
    PlanEntry e;
    RC(ensure(c, e.dev, nb + 16));
    if (nb) {
      hipError_t ce = hipMemcpy(e.dev.p, b, nb, hipMemcpyHostToDevice);
      if (ce != hipSuccess) {
        hipFree(e.dev.p);
        return fail(c, GS_ERR_DEVICE, "task table upload", ce);
      }
    }
    e.host.assign(b, b + nb);
    e.last_use = ++c->plan_clock;
    *out = (const T*)e.dev.p;
    c->plans.emplace(key, std::move(e));
    return GS_OK;
  }
}

// ---------------------------------------------------------------------------
// one side (G1 or G2) of commit / prove expressed as engine tasks
// ---------------------------------------------------------------------------
struct SidePlan {
  std::vector<GrpTask> grp;  // when tm > 1: lanes of k_var_multi (each sums <= tm consecutive var tasks)
  int tm = 1;
  int mo = 1, w = 4;  // outputs per lane after share_tables(), window width
  bool shared_done = false;
  std::vector<VarTask> var;
  std::vector<FixTask> fix;
  std::vector<RedTask> red;
  int nslots = 0;
  int ncom = 0;  // the first `ncom` reductions (the commitments) only sum fixed-base partial slots
  int tab_bases = 0;  // > 0: every variable-base term is over array 0, which holds this many bases per equation, and
                      // the side runs on shared per-base window tables (k_tab_build + k_var_tab) instead of Straus lanes
  bool points = false;  // the outputs are single points, not Com-shaped pairs: the reductions run k_red_pt
};

static FixTask mkfix(int s0, int t0, int s1, int t1, int a_arr, int a_idx, int slot, int a_neg = 0) {
  FixTask f;
  f.s0 = (uint32_t)s0;
  f.s1 = (uint32_t)s1;
  f.t0 = (uint8_t)t0;
  f.t1 = (uint8_t)t1;
  f.a_arr = (uint8_t)a_arr;
  f.a_idx = (uint32_t)a_idx;
  f.a_neg = (uint8_t)a_neg;
  f.slot = (uint32_t)slot;
  return f;
}
static VarTask mkvar(int s, int arr, int idx, int slot) {
  VarTask v;
  v.s_idx = (uint32_t)s;
  v.p_arr = (uint8_t)arr;
  v.p_idx = (uint32_t)idx;
  v.slot = (uint32_t)slot;
  v.neg = 0;
  v.pad0 = v.pad1 = 0;
  return v;
}
static RedTask mkred(int b0, int e0, int b1, int e1, int out_arr, int out_idx) {
  RedTask r;
  r.b0 = (uint32_t)b0;
  r.e0 = (uint32_t)e0;
  r.b1 = (uint32_t)b1;
  r.e1 = (uint32_t)e1;
  r.out_arr = (uint8_t)out_arr;
  r.out_idx = (uint32_t)out_idx;
  r.pad = r.pad1 = r.pad2 = 0;
  return r;
}
static void add_pair(std::vector<PairRef>& v, int p_arr, int p_idx, int neg, int q_arr, int q_idx) {
  PairRef r;
  r.p_arr = (uint8_t)p_arr;
  r.p_idx = (uint32_t)p_idx;
  r.neg = (uint8_t)neg;
  r.q_arr = (uint8_t)q_arr;
  r.q_idx = (uint32_t)q_idx;
  r.pad = 0;
  v.push_back(r);
}
// The Miller pairs of a verification equation, stated as FAMILIES of pairs (P_e, Q_e), e < count, between two sites.
// A site is element `el` onwards of array `arr`: Com-shaped (component c of element e is point 2 e + c) or bare points.
struct PairSite {
  int arr, el;
  bool com = true;
};
struct PairFamily {
  PairSite P, Q;
  int count;  // 0: the family is absent
  int neg;    // pair -P
};
// Appends (P_e.pc, Q_e.qc) for every family, in list order (the order fixes the task tables and which pairs share a
// lane).  A bare Q stands for iota(Q) = (O, Q): it only meets component 1.
static void add_pairs(std::vector<PairRef>& v, std::initializer_list<PairFamily> fams, int pc, int qc) {
  for (const PairFamily& f : fams) {
    if (!f.Q.com && qc != 1) continue;
    for (int e = 0; e < f.count; e++)
      add_pair(v, f.P.arr, 2 * (f.P.el + e) + pc, f.neg, f.Q.arr, f.Q.com ? 2 * (f.Q.el + e) + qc : f.Q.el + e);
  }
}
// An equation's shape: type and arity, and what the type says about each side (group-valued variables have two columns
// of commit randomness and two proof elements on the other side, scalars one)
struct Shape {
  int ty, m, n;
  bool xg, yg;
  int kx, ky;
  Shape(int ty_, int m_, int n_)
      : ty(ty_), m(m_), n(n_), xg(x_is_group(ty_)), yg(y_is_group(ty_)), kx(xg ? 2 : 1), ky(yg ? 2 : 1) {}
};
// What every verifier is given: the shape, the batch size (statements, for the Statement verifier) and the eight input
// arrays, in the order of the slots VI_A .. VI_TH
struct VerifyIn {
  Shape sh;
  size_t N;
  const void *A, *B, *G, *target, *xcoms, *ycoms, *pi, *theta;
  VerifyIn(int ty, size_t N_, int m, int n, const void* const* p)
      : sh(ty, m, n), N(N_), A(p[VI_A]), B(p[VI_B]), G(p[VI_G]), target(p[VI_TG]), xcoms(p[VI_XC]), ycoms(p[VI_YC]),
        pi(p[VI_PI]), theta(p[VI_TH]) {}
};
// A pool layout from its fields in pool order: pool_layout({{&PoolMap::GC, m * n}, ...}).  Fields that are not named
// stay zero.
struct PoolField {
  int PoolMap::*field;
  int count;
};
static PoolMap pool_layout(std::initializer_list<PoolField> fields) {
  PoolMap pm;
  memset(&pm, 0, sizeof pm);
  for (const PoolField& f : fields) {
    pm.*f.field = pm.total;
    pm.total += f.count;
  }
  return pm;
}
// An array table in one expression: arr_tab({{i, base, bytes per equation[, present]}, ...}).  Entries that are not
// named, or not present, stay zero.
struct ArrEnt {
  int i;
  const void* base;
  uint32_t stride;
  bool present = true;
};
static ArrTab arr_tab(std::initializer_list<ArrEnt> ents) {
  ArrTab t;
  memset(&t, 0, sizeof t);
  for (const ArrEnt& e : ents)
    if (e.present) {
      t.base[e.i] = (const uint8_t*)e.base;
      t.stride[e.i] = e.stride;
    }
  return t;
}
static OutTab out_tab(void* base0, uint32_t stride0, void* base1 = nullptr, uint32_t stride1 = 0) {
  OutTab t;
  memset(&t, 0, sizeof t);
  t.base[0] = (uint8_t*)base0;
  t.stride[0] = stride0;
  t.base[1] = (uint8_t*)base1;
  t.stride[1] = stride1;
  return t;
}

// Append the variable-base terms of ONE output point: chunks of <= tm terms share a lane
// (and one partial slot); with tm == 1 every term is its own lane/slot.
static void add_var_terms(SidePlan& sp, const std::vector<VarTask>& terms, int& slot) {
  size_t T = terms.size();
  if (T == 0) return;
  size_t tm = sp.tm < 1 ? 1 : (size_t)sp.tm, ng = (T + tm - 1) / tm, base = T / ng, rem = T % ng, s0 = 0;
  for (size_t k = 0; k < ng; k++) {  // balanced groups: sizes differ by <= 1
    size_t n = base + (k < rem ? 1 : 0);
    GrpTask g;
    memset(&g, 0, sizeof g);
    g.first[0] = (uint32_t)sp.var.size();
    g.nt = (uint32_t)n;
    g.no = 1;
    g.slot[0] = (uint32_t)slot;
    for (size_t i = 0; i < n; i++) {
      VarTask v = terms[s0 + i];
      v.slot = (uint32_t)slot;
      sp.var.push_back(v);
    }
    s0 += n;
    sp.grp.push_back(g);
    slot++;
  }
}
// Plans Com-shaped outputs (two components each).  The components of an output occupy consecutive runs of partial
// slots, in the order in which `emit(q, comp, out)` asks for them: out.fix(...) takes one slot for a fixed-base task
// (mkfix without its slot), out.terms(list) as many as add_var_terms gives the list.  A reduction over the two runs
// closes every output.
struct ComOutputs {
  SidePlan& sp;
  int slot = 0;
  void fix(int s0, int t0, int s1, int t1, int a_arr, int a_idx, int a_neg = 0) {
    sp.fix.push_back(mkfix(s0, t0, s1, t1, a_arr, a_idx, slot, a_neg));
    slot++;
  }
  void terms(const std::vector<VarTask>& t) { add_var_terms(sp, t, slot); }
  // outputs out0 .. out0 + count - 1 of array out_arr; emit's q runs from 0
  template <class Emit> void add(int count, int out_arr, int out0, Emit emit) {
    for (int q = 0; q < count; q++) {
      int b[2], e[2];
      for (int comp = 0; comp < 2; comp++) {
        b[comp] = slot;
        emit(q, comp, *this);
        e[comp] = slot;
      }
      sp.red.push_back(mkred(b[0], e[0], b[1], e[1], out_arr, out0 + q));
    }
    sp.nslots = slot;
  }
};
// ---- the G1 outputs of the verifiers, component b.  `pm` is the pool the lanes read: GC Gamma (m x n), BC b (m), and
// for the batched verifiers RH rho_ab at RH + 2 a + b, AR a_j rho_ab at AR + 4 j + 2 a + b, NR -t rho_ab likewise.
// sum_i s_i C_i.comp: scalars s0, s0 + stride, ..., the m Com-shaped elements of array `arr` (Gamma's column j, or b)
static void com_terms(std::vector<VarTask>& t, int s0, int stride, int m, int arr, int comp) {
  for (int i = 0; i < m; i++) t.push_back(mkvar(s0 + i * stride, arr, 2 * i + comp, 0));
}
// rho_0b K.0 + rho_1b K.1 for a CRS element K with tables t0, t1; the scalars (rho, a_j rho, -t rho) start at X
static void rho_fix(ComOutputs& o, int X, int b, int t0, int t1) { o.fix(X + b, t0, X + 2 + b, t1, 0xFF, 0); }
// rho_0b E.0 + rho_1b E.1 for element `idx` of array `arr` (C'_i from c_i, Th'_l from theta_l)
static void rho_comb(ComOutputs& o, const PoolMap& pm, int b, int arr, int idx) {
  o.terms({mkvar(pm.RH + b, arr, 2 * idx, 0), mkvar(pm.RH + 2 + b, arr, 2 * idx + 1, 0)});
}
// P'_j's head: rho_1b A_j (A = array arrA) as a term, or sum_a a_j rho_ab W1.a as a fixed-base lane
static void head_terms(ComOutputs& o, std::vector<VarTask>& t, const PoolMap& pm, const Shape& s, int j, int b, int arrA) {
  if (s.xg)
    t.push_back(mkvar(pm.RH + 2 + b, arrA, j, 0));
  else
    rho_fix(o, pm.AR + j * 4, b, tb_w(0), tb_w(1));
}
// PB'_b = sum_i b_i C'_ib [- rho_1b t] [- sum_a t rho_ab W1.a]  (C' = array arrC, t = array arrT)
static void emit_PB(ComOutputs& o, const PoolMap& pm, const Shape& s, int b, int arrC, int arrT) {
  std::vector<VarTask> terms;
  com_terms(terms, pm.BC, 1, s.m, arrC, b);
  if (s.ty == GS_MSMEG1) {
    VarTask v = mkvar(pm.RH + 2 + b, arrT, 0, 0);
    v.neg = 1;
    terms.push_back(v);
  }
  if (s.ty == GS_QUAD) rho_fix(o, pm.NR, b, tb_w(0), tb_w(1));
  o.terms(terms);
}
// U'_kb = rho_0b u_k.0 + rho_1b u_k.1 and W1'_b = rho_0b W1.0 + rho_1b W1.1
static void emit_U(ComOutputs& o, const PoolMap& pm, int k, int b) { rho_fix(o, pm.RH, b, tb_u(k, 0), tb_u(k, 1)); }
static void emit_W1(ComOutputs& o, const PoolMap& pm, int b) { rho_fix(o, pm.RH, b, tb_w(0), tb_w(1)); }
// one lane per final exponentiation once `items` of them fill the chip, 3-lane groups (21 per wave) below that
// (items: the launch's own count, or fillN of it where the launch can be a part of a mixed call)
static bool coop_lanes(const gs_ctx* c, size_t items) {
  return c->coop_fe == 2 || (c->coop_fe == 1 && (items + 20) / 21 <= c->simd_slots);
}
// Lane cost of the joint MSM in Fq multiplications: one table build of `nt` bases (2^(w-1) entries each: doublings,
// mixed additions, 7 multiplications per entry for the common denominator) + `no` main loops (w doublings per window,
// one mixed addition per non-zero digit, the endomorphism on the looked-up entry).
static double straus_lane_cost(bool g2, bool bn, int nt, int no, int w) {
  const double madd = g2 ? 29.0 : 11.0, dbl = g2 ? 16.0 : 8.0, gz = g2 ? 21.0 : 7.0, endo = g2 ? 4.0 : 0.5;
  const int ns = g2 ? 4 : 2, nl = g2 ? (bn ? 3 : 2) : (bn ? 5 : 4), nd = (32 * nl + w - 1) / w + 1, ne = 1 << (w - 1);
  double build = nt * (ne / 2 * dbl + (ne / 2 - 1) * madd + ne * gz);
  double run = (nd - 1) * w * dbl + (double)nt * ns * (nd - 0.5) * (1.0 - 1.0 / (2 * ne)) * (madd + endo);
  return build + no * run;
}
// Lane-time multiplier of a launch of `waves` waves.  The Fp2 / Fp12 kernels and the BLS12-381 G1 kernels hold one
// wave per SIMD: whole rounds while there are few.  The BN254 G1 Straus kernels come out of the compiler at 252
// registers and run two waves per SIMD; two resident waves finish in 2 / 1.55 of the time of one (measured at 2^16:
// k_var_multi8.g1 11.4 ms as 2048 waves against 16.7 ms as 1024 waves of twice the length).
static double wave_rounds(const gs_ctx* c, double waves, bool g2) {
  double r = waves / (double)c->simd_slots;
  if (g2 || c->curve != 1) {
    if (r <= 1.0) return 1.0;
    return r < 4.0 ? (double)(size_t)(r + 0.999) : r;
  }
  const double gain = 1.55;
  return r <= gain ? 1.0 : r / gain;
}
// Variable-base terms per lane (joint Straus MSM, shared doubling chain) for a side with `T` terms per output
// and `outputs` outputs per equation.  Same cost model as miller_cost: rounds of waves x lane length, lane(nt) =
// D + P nt Fq multiplications (fits of profiles/r1/fq_mul_counts.json, the same within 3 % on both curves now that
// both have endomorphism decompositions: G1 832 + 829 nt, G2 1000 + 2365 nt).
static int pick_tm(const gs_ctx* c, size_t N, int T, int outputs, bool g2, int share) {
  // `share` of the `outputs` run over the same bases (share_tables() can give them one table build per lane): the
  // group size is chosen together with the outputs per lane and the window width that share_tables() will then pick
  if (T < 2 || !c->endo) return 1;  // (no endomorphisms: one plain lane per term)
  if (c->var_tm > 0) {  // forced: the balanced group size is what runs
    int ng = (T + c->var_tm - 1) / c->var_tm;
    return (T + ng - 1) / ng;
  }
  int best_tm = 1;
  double best = -1;
  for (int tm = 1; tm <= 8; tm++) {
    int ng = (T + tm - 1) / tm, eff = (T + ng - 1) / ng;
    if (eff != tm) continue;  // the balanced size is what runs; skip aliases
    for (int mo : {1, 2, 4}) {
      if (mo > 1 && (eff < 2 || mo > share)) continue;  // one-term lanes are k_var: no sharing
      if (c->var_mo > 0 && mo != c->var_mo && !(eff < 2 && mo == 1)) continue;
      for (int w : {4, 5}) {
        if (w == 5 && eff < 2) continue;
        if (c->var_w > 0 && w != c->var_w && eff >= 2) continue;
        double lanes = (double)N * ((double)outputs / mo) * ng;
        double rounds = wave_rounds(c, lanes / 64.0, g2);
        // + the lane of k_red that folds the ng partial sums of an output (matters for large arities)
        double cost = rounds * straus_lane_cost(g2, c->curve == 1, eff, mo, w) +
                      fold_cost((double)ng, g2 ? 29.0 + 14.0 : 16.0);
        if (best < 0 || cost < best) {
          best = cost;
          best_tm = eff;
        }
      }
    }
  }
  return best_tm;
}

// Groups with the same bases (same arrays, indices and signs in the same order) become ONE lane of up to `mo` outputs
// that builds its tables once: the proof elements of a side share their constants and variables, the columns of
// Gamma^T c share the commitments.  Picks (mo, w) by the cost model of pick_tm unless overridden.
static void share_tables(const gs_ctx* c, size_t N, SidePlan& sp, bool g2) {
  if (sp.shared_done) return;
  sp.shared_done = true;
  sp.mo = 1;
  sp.w = 4;
  if (sp.tab_bases > 0) return;  // the lanes read the bases' shared tables: nothing to build per lane, one output each
  if (sp.tm <= 1 || sp.grp.empty()) return;
  // families of groups over the same bases, in plan order: hash of (nt, (index, array, sign) of every base), with
  // the bases compared on a hash match (large arities have ~10^5 groups: no strings, no ordered map)
  auto same = [&](const GrpTask& a, const GrpTask& b) {
    if (a.nt != b.nt) return false;
    for (uint32_t i = 0; i < a.nt; i++) {
      const VarTask &x = sp.var[a.first[0] + i], &y = sp.var[b.first[0] + i];
      if (x.p_idx != y.p_idx || x.p_arr != y.p_arr || x.neg != y.neg) return false;
    }
    return true;
  };
  std::vector<std::vector<size_t>> fam;
  std::unordered_map<uint64_t, std::vector<size_t>> by_hash;  // hash -> families
  int ntmax = 1;
  for (size_t i = 0; i < sp.grp.size(); i++) {
    const GrpTask& g = sp.grp[i];
    uint64_t h = 1469598103934665603ull ^ g.nt;
    for (uint32_t k = 0; k < g.nt; k++) {
      const VarTask& v = sp.var[g.first[0] + k];
      h = (h ^ (((uint64_t)v.p_idx << 16) | ((uint64_t)v.p_arr << 8) | v.neg)) * 1099511628211ull;
    }
    std::vector<size_t>& cand = by_hash[h];
    size_t f = (size_t)-1;
    for (size_t c2 : cand)
      if (same(sp.grp[fam[c2][0]], g)) {
        f = c2;
        break;
      }
    if (f == (size_t)-1) {
      f = fam.size();
      fam.emplace_back();
      cand.push_back(f);
    }
    fam[f].push_back(i);
    ntmax = std::max(ntmax, (int)g.nt);
  }
  size_t share = 1;
  for (auto& f : fam) share = std::max(share, f.size());
  int best_mo = 1, best_w = 4;
  double best = -1;
  for (int mo : {1, 2, 4}) {
    if (c->var_mo > 0 && mo != c->var_mo) continue;
    if (c->var_mo <= 0 && (size_t)mo > share) continue;
    size_t lanes = 0;
    for (auto& f : fam) lanes += (f.size() + mo - 1) / mo;
    for (int w : {4, 5}) {
      if (c->var_w > 0 && w != c->var_w) continue;
      // a part of a mixed call: one window width for every part, or their Straus lanes are two kernel instances and go
      // out as two under-filled launches (2^12 mixed: 3.1 + 4.7 ms where one launch takes 4.7)
      if (c->var_w <= 0 && c->rec && w != 4) continue;
      double rounds = wave_rounds(c, (double)N * lanes / 64.0, g2);
      int eff_mo = (int)std::min((size_t)mo, share);
      double cost = rounds * straus_lane_cost(g2, c->curve == 1, ntmax, eff_mo, w);
      if (best < 0 || cost < best) {
        best = cost;
        best_mo = mo;
        best_w = w;
      }
    }
  }
  sp.mo = best_mo;
  sp.w = best_w;
  if (getenv("GS_PLAN_TRACE")) {
    size_t lanes = 0;
    for (auto& f : fam) lanes += (f.size() + best_mo - 1) / best_mo;
    fprintf(stderr, "[plan] straus %s fill %zu: %zu groups in %zu families (largest %zu), <= %d terms; outputs per build %d, window %d, "
            "%zu lanes per equation\n", g2 ? "G2" : "G1", N, sp.grp.size(), fam.size(), share, ntmax, best_mo, best_w, lanes);
  }
  if (best_mo == 1) return;
  std::vector<GrpTask> merged;
  for (const std::vector<size_t>& f : fam) {
    for (size_t b = 0; b < f.size(); b += best_mo) {
      GrpTask g = sp.grp[f[b]];
      g.no = (uint32_t)std::min((size_t)best_mo, f.size() - b);
      for (uint32_t o = 1; o < g.no; o++) {
        g.first[o] = sp.grp[f[b + o]].first[0];
        g.slot[o] = sp.grp[f[b + o]].slot[0];
      }
      merged.push_back(g);
    }
  }
  sp.grp.swap(merged);
}

// Build the plan of one side.
//  nv      committed variables on this side (m for the G1 side, n for the G2 side)
//  nc      constants paired with the OTHER side's variables that live here (len of A for G1 side = n; B for G2 = m)
//  group   variables on this side are group elements (else scalars)
//  kc      columns of this side's commit randomness (2 group / 1 scalar)
//  npf     number of proof elements on this side (theta count = ky for G1 side, pi count = kx for G2 side)
//  offsets into the pool: rc (nv x kc commit randomness), vc (scalar variables), cs (nc x npf scalars multiplying
//  the constants: SC for the G1 side / RC for the G2 side, indexed [j*npf + l]), ph (npf x nv: PHI / PSI),
//  f0 (npf x kc fixed scalars: TC for G1 side, OM for G2 side), sg (npf: SIG / RHO)
//  arrays: 0 = variables (group), 1 = constants (group)
static void build_side(SidePlan& sp, bool want_coms, int nv, int nc, bool group, int kc, int npf, int rc, int vc,
                       int cs, int ph, int f0, int sg) {
  ComOutputs out{sp};
  if (want_coms) {
    out.add(nv, 0, 0, [&](int i, int c, ComOutputs& o) {
      if (group)
        o.fix(rc + 2 * i, tb_u(0, c), rc + 2 * i + 1, tb_u(1, c), c ? 0 : 0xFF, i);
      else
        o.fix(vc + i, tb_w(c), rc + i, tb_u(0, c), 0xFF, 0);
    });
    sp.ncom = nv;
  }
  out.add(npf, 1, 0, [&](int l, int c, ComOutputs& o) {
    if (!group) return o.fix(sg + l, tb_w(c), f0 + l, tb_u(0, c), 0xFF, 0);
    o.fix(f0 + l * 2, tb_u(0, c), f0 + l * 2 + 1, tb_u(1, c), 0xFF, 0);
    if (c == 0) return;  // iota(const) = (O, const), and the variables enter through component 1 alone
    std::vector<VarTask> terms;
    for (int j = 0; j < nc; j++) terms.push_back(mkvar(cs + j * npf + l, 1, j, 0));
    for (int i = 0; i < nv; i++) terms.push_back(mkvar(ph + l * nv + i, 0, i, 0));
    o.terms(terms);
  });
}

// Build the plan of one side of a RERANDOMIZATION (no witness: the variables are known only through their old
// commitments, which enter as variable-base terms -- both components of each -- and as affine addends).
//  nv, nc, group, kc, npf   as in build_side; npf = 0 plans the commitments alone (a Statement's, made once)
//  pool offsets: rc (nv x kc fresh commit randomness), cs (nc x npf: S' for the G1 side / R' for the G2 side, [j*npf + l]),
//  ph (npf x nv: PHI' / PSI'), f0 (npf x kc: T' / OMEGA'), sg (npf: SIG' = S'^T a / RHO' = R'^T b, scalar sides)
//  arrays: 0 = old commitments (2 nv points: component c of commitment i is point 2 i + c), 1 = constants (group),
//  2 = old proof elements (2 npf points)
//    com'_i.c   = com_i.c + sum_a rand_ia key_a.c                                  (fixed + addend)
//    pf'_l.c    = pf_l.c + f0_l . key.c [+ sg_l W.c] + sum_i ph_li com_i.c [+ (c = 1) sum_j cs_jl const_j]
static void build_rerand_side(SidePlan& sp, bool want_coms, int nv, int nc, bool group, int kc, int npf, int rc, int cs,
                              int ph, int f0, int sg) {
  ComOutputs out{sp};
  if (want_coms) {
    out.add(nv, 0, 0, [&](int i, int c, ComOutputs& o) {
      if (group)
        o.fix(rc + 2 * i, tb_u(0, c), rc + 2 * i + 1, tb_u(1, c), 0, 2 * i + c);
      else
        o.fix(rc + i, tb_u(0, c), 0, 0xFF, 0, 2 * i + c);
    });
    sp.ncom = nv;
  }
  out.add(npf, 1, 0, [&](int l, int c, ComOutputs& o) {
    if (group)
      o.fix(f0 + l * 2, tb_u(0, c), f0 + l * 2 + 1, tb_u(1, c), 2, 2 * l + c);
    else
      o.fix(sg + l, tb_w(c), f0 + l, tb_u(0, c), 2, 2 * l + c);
    std::vector<VarTask> terms;
    if (group && c == 1)  // iota(const) = (O, const)
      for (int j = 0; j < nc; j++) terms.push_back(mkvar(cs + j * npf + l, 1, j, 0));
    for (int i = 0; i < nv; i++) terms.push_back(mkvar(ph + l * nv + i, 0, 2 * i + c, 0));
    o.terms(terms);
  });
}

// the reduction launch of a side, kept back so that the caller can run the two sides' reductions side by side
struct RedLaunch {
  std::string name, tag;
  std::vector<RedTask> hred;  // host copy: long runs are folded in parallel first (run_red)
  const void* part = nullptr;
  size_t nred = 0;
  int nslots = 0;
  OutTab outs;
  bool points = false;  // one point per output (k_red_pt)
};
constexpr uint32_t RED_FOLD_K = 8, RED_RUN_MAX = 16;
template <class C, class F> static int run_red(gs_ctx* c, size_t N, const RedLaunch& r) {
  std::vector<RedTask> red = r.hred;
  const Jac<F>* part = (const Jac<F>*)r.part;
  int nslots = r.nslots;
  // segmented K-ary tree: while a component of some output still sums more than RED_RUN_MAX slots, fold runs of K
  for (int level = 0;; level++) {
    uint32_t longest = 0;
    for (const RedTask& t : red) {
      longest = std::max(longest, t.e0 - t.b0);
      longest = std::max(longest, t.e1 - t.b1);
    }
    if (longest <= RED_RUN_MAX) break;
    std::vector<FoldTask> ft;
    uint32_t next = 0;
    auto fold_range = [&](uint32_t& b, uint32_t& e) {
      uint32_t nb = next;
      for (uint32_t lo = b; lo < e; lo += RED_FOLD_K) ft.push_back(FoldTask{lo, std::min(lo + RED_FOLD_K, e), next++, 0});
      b = nb;
      e = next;
    };
    for (RedTask& t : red) {
      fold_range(t.b0, t.e0);
      fold_range(t.b1, t.e1);
    }
    const FoldTask* dft;
    RC(upload(c, (r.tag + ".fold").c_str(), ft, &dft));
    void* out;
    RC(scratch(c, (r.tag + (level & 1 ? ".fold1" : ".fold0")).c_str(), N * (size_t)next * sizeof(Jac<F>), &out));
    c->work_hint = N * (uint64_t)nslots;
    RC(launch_seg<k_slot_fold<C, F>>(c, (std::string("k_slot_fold") + r.tag).c_str(), N * ft.size(), 64, N * ft.size(),
              (int)ft.size(), dft, part, nslots, (Jac<F>*)out, (int)next));
    part = (const Jac<F>*)out;
    nslots = (int)next;
  }
  const RedTask* dred;
  RC(upload(c, (r.tag + ".red").c_str(), red, &dred));
  c->work_hint = N * (uint64_t)nslots;  // partial sums folded
  // outputs per lane (one inversion each lane): as many as still leave the launch a full round of waves
  int K = 1;
  // (K may exceed the outputs of an equation: 6 outputs go to ONE lane of 8 rather than to lanes of 4 + 2 with an
  // inversion each, once a lane per equation still fills the chip)
  while (K < RED_K && K < (int)r.nred && (fillN(c, N) * ((r.nred + 2 * K - 1) / (2 * K)) + 63) / 64 >= c->simd_slots) K *= 2;
  if (c->red_k > 0) K = std::min(c->red_k, RED_K);
  size_t lanes = N * ((r.nred + K - 1) / K);
  if (r.points)
    return launch_seg<k_red_pt<C, F>>(c, r.name.c_str(), lanes, 64, lanes, (int)r.nred, dred, part, nslots, r.outs, K);
  return launch_seg<k_red<C, F>>(c, r.name.c_str(), lanes, 64, lanes, (int)r.nred, dred, part, nslots, r.outs, K);
}
template <class C, class F>
static int run_side(gs_ctx* c, const char* tag, size_t N, SidePlan& sp, const ArrTab& arrs, const Fr<C>* pool,
                    int pool_n, const Aff<F>* tab, const OutTab& outs, hipStream_t vstream = nullptr,
                    hipEvent_t vev0 = nullptr, hipEvent_t vev1 = nullptr, const unsigned* pipe_masks = nullptr) {
  // pipe_masks (host-pointer calls): {inputs the fixed-base kernel reads, inputs the variable-base kernel reads,
  // outputs complete after the commitments' reduction, outputs complete after the side's last reduction}
  std::string t(tag);
  share_tables(c, fillN(c, N), sp, std::is_same<F, Fp2<C>>::value);
  const VarTask* dvar;
  const FixTask* dfix;
  RC(upload(c, (t + ".var").c_str(), sp.var, &dvar));
  RC(upload(c, (t + ".fix").c_str(), sp.fix, &dfix));
  void* part;
  RC(scratch(c, (t + ".part").c_str(), N * sp.nslots * sizeof(Jac<F>), &part));
  // fork: the variable-base kernel goes to `vstream` (if any) while the fixed-base one stays on the side's stream
  hipStream_t base = c->cur ? c->cur : c->stream;
  bool fork = vstream != nullptr && !c->prof;
  if (fork) {
    hipEventRecord(vev0, base);
    hipStreamWaitEvent(vstream, vev0, 0);
  }
  if (pipe_masks) RC(need(c, pipe_masks[0]));
  {
    uint64_t terms = 0;  // fixed-base scalars per equation
    for (const FixTask& f : sp.fix) terms += (f.t0 != 0xFF) + (f.t1 != 0xFF);
    c->work_hint = N * terms;
  }
  RC(launch_seg<k_fix<C, F>>(c, (std::string("k_fix") + tag).c_str(), N * sp.fix.size(), 64, N * sp.fix.size(),
            (int)sp.fix.size(), dfix, arrs, pool, pool_n, tab, (Jac<F>*)part, sp.nslots));
  // host-pointer calls: the commitments depend on the fixed-base kernel alone -- reduce them now and send them back
  // across PCIe under the variable-base kernel
  // (from 2^14 equations on: below that the extra launch and events cost more than the copy they hide)
  const bool early = c->pipe && pipe_masks && !c->rec && !fork && sp.ncom > 0 && sp.ncom < (int)sp.red.size() &&
                     N >= 16 * c->simd_slots;
  if (early) {
    RedLaunch rc0;
    rc0.name = std::string("k_red") + tag;
    rc0.tag = t + ".coms";
    rc0.hred.assign(sp.red.begin(), sp.red.begin() + sp.ncom);
    rc0.part = part;
    rc0.nred = (size_t)sp.ncom;
    rc0.nslots = sp.nslots;
    rc0.outs = outs;
    RC((run_red<C, F>(c, N, rc0)));
    RC(out_ready(c, pipe_masks[2]));
  }
  if (fork) c->cur = vstream;
  // (the variable-base kernel reads the variables too, and on a forked stream nothing has waited for them yet)
  if (pipe_masks) RC(need(c, pipe_masks[0] | pipe_masks[1]));
  if (sp.tab_bases > 0) {
    // shared per-base window tables (8-bit signed windows: 128 affine multiples per base), then Straus-shaped lanes of
    // up to 8 terms that only read them
    constexpr int TW = 8, TNE = 1 << (TW - 1);
    const size_t nbt = N * (size_t)sp.tab_bases;
    void *tabs, *stage;
    RC(scratch(c, (t + ".tab8").c_str(), nbt * TNE * sizeof(Aff<F>), &tabs));
    RC(scratch(c, (t + ".tab8j").c_str(), nbt * TNE * sizeof(Jac<F>), &stage));
    c->work_hint = nbt;
    RC((launch_seg<k_tab_build<C, F, TW>>(c, (std::string("k_tab_build") + tag).c_str(), nbt, 64, nbt, sp.tab_bases, arrs, 0,
                                          (Jac<F>*)stage, (Aff<F>*)tabs)));
    const GrpTask* dgrp;
    RC(upload(c, (t + ".grp").c_str(), sp.grp, &dgrp));
    const size_t tot = N * sp.grp.size();
    c->work_hint = N * sp.var.size();  // terms
    RC((launch_seg<k_var_tab<C, F, 8, TW>>(c, (std::string("k_var_tab8") + tag).c_str(), tot, 64, tot, (int)sp.grp.size(), dgrp,
                                           dvar, pool, pool_n, (Jac<F>*)part, sp.nslots, (const Aff<F>*)tabs, sp.tab_bases)));
  } else if (sp.tm <= 1 && !c->endo) {
    RC((launch_seg<k_var<C, F, false>>(c, (std::string("k_var.plain") + tag).c_str(), N * sp.var.size(), 64, N * sp.var.size(),
              (int)sp.var.size(), dvar, arrs, pool, pool_n, (Jac<F>*)part, sp.nslots)));
  } else if (sp.tm <= 1) {
    RC(launch_seg<k_var<C, F>>(c, (std::string("k_var") + tag).c_str(), N * sp.var.size(), 64, N * sp.var.size(),
              (int)sp.var.size(), dvar, arrs, pool, pool_n, (Jac<F>*)part, sp.nslots));
  } else {
    const GrpTask* dgrp;
    RC(upload(c, (t + ".grp").c_str(), sp.grp, &dgrp));
    size_t tot = N * sp.grp.size();
    c->work_hint = N * sp.var.size();  // terms
    // the lanes' Straus tables: lane-contiguous global workspace (see jac_msm_straus_at), at most VAR_WS_LANES lanes
    // of it; a larger batch goes in several launches over the same workspace
    // (parts of a mixed call share a launch when they agree on the instance: the window width is fixed for them in
    // share_tables; the 4- or 8-term instance follows the part's own group size -- the 8-term one runs 4-term groups
    // too, but 1.8x slower (2^12 mixed: 5.6 against 3.1 ms), so parts are not forced onto it)
    const int tmax = sp.tm > 4 ? 8 : 4;
    const size_t lane_ws = ((size_t)tmax << (sp.w - 1)) * (sizeof(Aff<F>) + sizeof(Jac<F>));
    // (the buffer is grow-only: a workspace that already holds more lanes is used as it is)
    size_t have = 0;
    {
      auto it = c->scratch.find((c->scratch_tag ? "m" + std::to_string(c->scratch_tag) + ":" : std::string()) + t + ".tabws");
      if (it != c->scratch.end()) have = it->second.cap / lane_ws;
    }
    const size_t chunk = std::min(tot, c->var_ws_lanes > 0 ? (size_t)c->var_ws_lanes
                                                            : std::max(std::min(have, tot), var_ws_auto(c, tot, lane_ws)));
    void* tabws;
    RC(scratch(c, (t + ".tabws").c_str(), chunk * lane_ws, &tabws));
    // kernel name: k_var_multi<TMAX>[w5][x<outputs per lane>]
    std::string kn = std::string("k_var_multi") + (tmax == 4 ? "4" : "8") + (sp.w == 5 ? "w5" : "") +
                     (sp.mo > 1 ? "x" + std::to_string(sp.mo) : "") + tag;
    for (size_t g0 = 0; g0 < tot; g0 += chunk) {
      size_t n = std::min(chunk, tot - g0);
      c->work_hint = (uint64_t)((double)N * sp.var.size() * ((double)n / (double)tot));  // terms
      // G1 lanes in the two-waves-per-SIMD build when the launch puts (nearly) two waves on every SIMD: fewer, and the
      // dispatcher doubles waves up on some SIMDs while others idle (measured in round 2: 27 ms instead of 17.7)
      // MEASURED (round 4, gpurun_out/r4h): the verifier's 2048-wave launch at 2^16 takes 28.85 ms in the two-wave
      // build against 29.07 ms in the one-wave build -- the multiply-add pipe is quarter rate whoever issues into
      // it, and the 256-register build pays for the waits it hides with spills.  Kept as a forced shape (var_w2 = 1),
      // never planned.
      const bool w2 = std::is_same<F, Fq<C>>::value && c->var_w2 == 1;
#define GS_VM(TM, WW)                                                                                                \
  do {                                                                                                               \
    if (w2)                                                                                                          \
      RC((launch_seg<k_var_multi<C, F, TM, WW, (std::is_same<F, Fq<C>>::value ? 2 : 1)>>(                            \
          c, kn.c_str(), n, 64, tot, (int)sp.grp.size(), dgrp, dvar, arrs, pool, pool_n, (Jac<F>*)part, sp.nslots, g0, \
          (Aff<F>*)tabws)));                                                                                         \
    else                                                                                                             \
      RC((launch_seg<k_var_multi<C, F, TM, WW>>(c, kn.c_str(), n, 64, tot, (int)sp.grp.size(), dgrp, dvar, arrs, pool, \
                                                pool_n, (Jac<F>*)part, sp.nslots, g0, (Aff<F>*)tabws)));              \
  } while (0)
      if (tmax == 4 && sp.w == 5)
        GS_VM(4, 5);
      else if (tmax == 4)
        GS_VM(4, 4);
      else if (sp.w == 5)
        GS_VM(8, 5);
      else
        GS_VM(8, 4);
#undef GS_VM
    }
  }
  if (fork) {  // join before the reduction
    hipEventRecord(vev1, vstream);
    c->cur = base == c->stream ? nullptr : base;
    hipStreamWaitEvent(base, vev1, 0);
  }
  RedLaunch r;
  r.name = std::string("k_red") + tag;
  r.tag = t;
  if (early)
    r.hred.assign(sp.red.begin() + sp.ncom, sp.red.end());
  else
    r.hred = sp.red;
  r.part = part;
  r.nred = r.hred.size();
  r.nslots = sp.nslots;
  r.outs = outs;
  r.points = sp.points;
  RC((run_red<C, F>(c, N, r)));
  if (pipe_masks) RC(out_ready(c, pipe_masks[2] | pipe_masks[3]));
  return GS_OK;
}

// ---------------------------------------------------------------------------
// per-curve implementation
// ---------------------------------------------------------------------------
template <class C> struct Impl {
  typedef Fq<C> F1;
  typedef Fp2<C> F2;
  typedef Aff<F1> A1;
  typedef Aff<F2> A2;
  typedef Fr<C> S;
  typedef Fp12<C> GT;
  typedef Sz<C> Z;

  static int set_crs(gs_ctx* c, const void* crs_host) {
    const uint8_t* h = (const uint8_t*)crs_host;
    // an identical CRS already installed on this device (by any context of the process)?  share its tables
    {
      std::lock_guard<std::mutex> lk(g_tables_mu);
      for (auto it = g_tables.begin(); it != g_tables.end();) {
        std::shared_ptr<CrsTables> t = it->lock();
        if (!t) {
          it = g_tables.erase(it);
          continue;
        }
        if (t->device == c->device && t->curve == c->curve && t->crs_bytes.size() == Z::CRS &&
            memcmp(t->crs_bytes.data(), h, Z::CRS) == 0) {
          c->tabs = t;
          c->have_crs = true;
          return GS_OK;
        }
        ++it;
      }
    }
    std::shared_ptr<CrsTables> tb = std::make_shared<CrsTables>();
    tb->device = c->device;
    tb->curve = c->curve;
    tb->crs_bytes.assign(h, h + Z::CRS);
    c->have_crs = false;
    c->tabs = tb;  // (a failed build leaves have_crs false; the tables die with the last reference)
    // device copies (boundary form): 6 G1 points u0.0 u0.1 u1.0 u1.1 W1.0 W1.1, same for G2
    std::vector<uint8_t> g1pts(6 * Z::G1), g2pts(6 * Z::G2);
    memcpy(&g1pts[0], h, 4 * Z::G1);
    memcpy(&g2pts[0], h + 2 * Z::COM1, 4 * Z::G2);
    const uint8_t* g1 = h + 2 * Z::COM1 + 2 * Z::COM2;
    const uint8_t* g2 = g1 + Z::G1;
    // W1 = u[1] + (O, g1), W2 = v[1] + (O, g2)   (data_structures.rs:323-326, 368-371), derived on the device:
    // slot 4 = u1.0, slot 5 holds the addend on the way in
    memcpy(&g1pts[4 * Z::G1], &g1pts[2 * Z::G1], Z::G1);
    memcpy(&g2pts[4 * Z::G2], &g2pts[2 * Z::G2], Z::G2);
    memcpy(&g1pts[5 * Z::G1], g1, Z::G1);
    memcpy(&g2pts[5 * Z::G2], g2, Z::G2);
    RC(ensure(c, tb->crs_g1, g1pts.size()));
    RC(ensure(c, tb->crs_g2, g2pts.size()));
    HIPCHK(c, hipMemcpy(tb->crs_g1.p, g1pts.data(), g1pts.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(tb->crs_g2.p, g2pts.data(), g2pts.size(), hipMemcpyHostToDevice));
    RC(launch(c, "k_crs_derive.g1", k_crs_derive<C, F1>, 1, 64, (uint8_t*)tb->crs_g1.p));
    RC(launch(c, "k_crs_derive.g2", k_crs_derive<C, F2>, 1, 64, (uint8_t*)tb->crs_g2.p));
    // Miller line tables of the six G2 points (v0, v1, W2): the verifier pairs theta / PB against them
    RC(ensure(c, tb->line_tab, 6 * (size_t)miller_line_count<C>() * sizeof(Line<C>)));
    RC(launch(c, "k_line_tables", k_line_tables<C>, 6, 64, (const uint8_t*)tb->crs_g2.p, (Line<C>*)tb->line_tab.p));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(g1pts.data(), tb->crs_g1.p, g1pts.size(), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(g2pts.data(), tb->crs_g2.p, g2pts.size(), hipMemcpyDeviceToHost));
    // window tables (internal form) for bases {u0.0,u0.1,u1.0,u1.1,W.1}
    std::vector<uint8_t> b1(5 * Z::G1), b2(5 * Z::G2);
    memcpy(&b1[0], &g1pts[0], 4 * Z::G1);
    memcpy(&b1[4 * Z::G1], &g1pts[5 * Z::G1], Z::G1);
    memcpy(&b2[0], &g2pts[0], 4 * Z::G2);
    memcpy(&b2[4 * Z::G2], &g2pts[5 * Z::G2], Z::G2);
    void *db1, *db2;
    RC(scratch(c, "crs.b1", b1.size(), &db1));
    RC(scratch(c, "crs.b2", b2.size(), &db2));
    HIPCHK(c, hipMemcpy(db1, b1.data(), b1.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(db2, b2.data(), b2.size(), hipMemcpyHostToDevice));
    // first-level (8-bit) window tables only feed k_build_tables16: context scratch, reused by the next CRS
    size_t ne = (size_t)5 * 32 * 256;
    void *t8g1, *t8g2;
    RC(scratch(c, "crs.tab8.g1", ne * sizeof(A1), &t8g1));
    RC(scratch(c, "crs.tab8.g2", ne * sizeof(A2), &t8g2));
    RC(launch(c, "k_build_tables.g1", k_build_tables<C, F1>, ne, 64, 5, (const uint8_t*)db1, (A1*)t8g1));
    RC(launch(c, "k_build_tables.g2", k_build_tables<C, F2>, ne, 64, 5, (const uint8_t*)db2, (A2*)t8g2));
    size_t ne16 = (size_t)5 * 16 * 65536;
    RC(ensure(c, tb->tab16_g1, ne16 * sizeof(A1)));
    RC(ensure(c, tb->tab16_g2, ne16 * sizeof(A2)));
    RC(launch(c, "k_build_tables16.g1", k_build_tables16<C, F1>, ne16 / 16, 64, 5, (const A1*)t8g1, (A1*)tb->tab16_g1.p));
    RC(launch(c, "k_build_tables16.g2", k_build_tables16<C, F2>, ne16 / 16, 64, 5, (const A2*)t8g2, (A2*)tb->tab16_g2.p));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    {
      std::lock_guard<std::mutex> lk(g_tables_mu);
      g_tables.push_back(tb);
    }
    c->have_crs = true;
    return GS_OK;
  }

  static PoolMap prove_pool(int m, int n, int kx, int ky) {
    return pool_layout({{&PoolMap::RC, m * kx}, {&PoolMap::SC, n * ky}, {&PoolMap::PSI, kx * n}, {&PoolMap::PHI, ky * m},
                        {&PoolMap::OM, kx * ky}, {&PoolMap::TC, ky * kx}, {&PoolMap::RHO, kx}, {&PoolMap::SIG, ky},
                        {&PoolMap::XC, m}, {&PoolMap::YC, n}});
  }

  // The prover's scalar preparation into `pool`, launched as `name` (large arities: `name`.a and .b, one lane per
  // output scalar).  xs / ys: scalar witnesses, as / bs: scalar constants; null where that side is group-valued or
  // (rerandomization) there is no witness.
  static int prep_prove(gs_ctx* c, const std::string& name, size_t N, int m, int n, int kx, int ky, const void* G,
                        const void* R, const void* Sm, const void* T, const void* xs, const void* ys, const void* as,
                        const void* bs, const PoolMap& pm, void* pool, bool shared) {
    if (wide_prep(m, n)) {
      int W = m * kx + n * ky + ky * kx + m + n + kx * n + ky * m;
      RC(launch_seg<k_prep_prove_wide_a<C>>(c, (name + ".a").c_str(), N * (size_t)W, 64, N * (size_t)W, W, m, n, kx, ky,
                (const S*)G, (const S*)R, (const S*)Sm, (const S*)T, (const S*)xs, (const S*)ys, pm, (S*)pool,
                shared ? 1 : 0));
      size_t tb = N * (size_t)(kx * ky + kx + ky);
      return launch_seg<k_prep_prove_wide_b<C>>(c, (name + ".b").c_str(), tb, 64, tb, m, n, kx, ky, (const S*)R,
                (const S*)Sm, (const S*)T, (const S*)xs, (const S*)ys, (const S*)as, (const S*)bs, pm, (S*)pool,
                shared ? 1 : 0);
    }
    return launch_seg<k_prep_prove<C>>(c, name.c_str(), N, 64, N, m, n, kx, ky, (const S*)G, (const S*)R, (const S*)Sm,
              (const S*)T, (const S*)xs, (const S*)ys, (const S*)as, (const S*)bs, pm, (S*)pool, shared ? 1 : 0);
  }

  // prove / commit_and_prove for all four types (prove.rs:71-489)
  // shared: a Statement -- the N equations are over the SAME variables X, Y and commit randomness R, S (one copy,
  // stride 0); constants, Gamma, T and the proofs stay per equation.  Commitments are then made once by the caller.
  static int prove(gs_ctx* c, int ty, size_t N, int m, int n, const void* X, const void* Y, const void* A,
                   const void* B, const void* G, const void* R, const void* Sm, const void* T, void* xcoms,
                   void* ycoms, void* pi, void* theta, bool shared = false) {
    const Shape sh(ty, m, n);
    PoolMap pm = prove_pool(m, n, sh.kx, sh.ky);
    void* pool;
    RC(scratch(c, "prove.pool", N * pm.total * sizeof(S), &pool));
    RangeGuard rg_all("gs.prove");
    // (host-pointer calls: the scalars first; group-valued variables and constants are not read before their side)
    RC(need(c, BIT(PI_G) | BIT(PI_R) | BIT(PI_S) | BIT(PI_T) | (sh.xg ? 0u : BIT(PI_X) | BIT(PI_A)) |
                   (sh.yg ? 0u : BIT(PI_Y) | BIT(PI_B))));
    RC(prep_prove(c, "k_prep_prove", N, m, n, sh.kx, sh.ky, G, R, Sm, T, sh.xg ? nullptr : X, sh.yg ? nullptr : Y,
                  sh.xg ? nullptr : A, sh.yg ? nullptr : B, pm, pool, shared));
    // small batches: G1 side on the context's stream, G2 side on side[0], each side's variable-base kernel on a
    // further stream; everything joins back before this function returns
    struct CurGuard {
      gs_ctx* c;
      ~CurGuard() { c->cur = nullptr; }
    } guard{c};
    // (measured: +18 % at 2^10, but -4 % at 2^12 where each variable-base kernel already fills the SIMDs, so only
    // while a side's variable-base lanes occupy at most half of them)
    const bool ov = c->overlap && !c->prof && !c->rec && c->side[0] && fillN(c, N) * (size_t)(m + n) * 2 <= 32 * c->simd_slots;
    if (ov) {
      hipEventRecord(c->sev[0], c->stream);
      hipStreamWaitEvent(c->side[0], c->sev[0], 0);
    }
    // (larger batches once ran the two sides' reduction kernels side by side on a second stream: +1-2 % at 2^12..2^16,
    // but the extra queue's scratch reservation cost later big kernels 4x -- profiles/r3/scratch_pool.txt.  Removed.)
    // G1 side: xcoms (m) + theta (ky).  constants A (len n) multiply S; Phi multiplies X; fixed part T.
    // G2 side: ycoms (n) + pi (kx).  constants B (len m) multiply R; Psi multiplies Y; fixed part Omega.
    auto side = [&](auto* ftag) -> int {
      typedef std::remove_pointer_t<decltype(ftag)> F;
      constexpr bool g2 = std::is_same<F, F2>::value;
      const bool grp = g2 ? sh.yg : sh.xg;
      const int nv = g2 ? n : m, nc = g2 ? m : n, kc = g2 ? sh.ky : sh.kx, npf = g2 ? sh.kx : sh.ky;
      const size_t zp = g2 ? Z::G2 : Z::G1;
      void* coms = g2 ? ycoms : xcoms;
      SidePlan sp;
      sp.tm = grp ? pick_tm(c, fillN(c, N), m + n, npf, g2, npf) : 1;
      if (g2)
        build_side(sp, coms != nullptr, nv, nc, grp, kc, npf, pm.SC, pm.YC, pm.RC, pm.PSI, pm.OM, pm.RHO);
      else
        build_side(sp, coms != nullptr, nv, nc, grp, kc, npf, pm.RC, pm.XC, pm.SC, pm.PHI, pm.TC, pm.SIG);
      const ArrTab arrs = arr_tab({{0, g2 ? Y : X, shared ? 0u : (uint32_t)(nv * zp), grp},
                                   {1, g2 ? B : A, (uint32_t)(nc * zp), grp}});
      const OutTab outs = out_tab(coms, (uint32_t)(nv * 2 * zp), g2 ? pi : theta, (uint32_t)(npf * 2 * zp));
      if (g2 && ov) c->cur = c->side[0];  // the whole G2 side runs beside the G1 side
      RangeGuard rg(g2 ? "gs.prove.g2" : "gs.prove.g1");
      // (the fixed-base kernel reads the variables as the commitments' affine addend; the constants only feed the
      // variable-base one)
      const unsigned masks[4] = {BIT(g2 ? PI_Y : PI_X), BIT(g2 ? PI_B : PI_A), BIT(g2 ? PO_YC : PO_XC),
                                 BIT(g2 ? PO_PI : PO_TH)};
      const void* tab = g2 ? c->tabs->tab16_g2.p : c->tabs->tab16_g1.p;
      // the side's variable-base kernel forks to side[1] (events 1, 2) on G1, to side[2] (events 3, 4) on G2
      RC((run_side<C, F>(c, g2 ? ".g2" : ".g1", N, sp, arrs, (const S*)pool, pm.total, (const Aff<F>*)tab, outs,
                         ov ? c->side[g2 ? 2 : 1] : nullptr, c->sev[g2 ? 3 : 1], c->sev[g2 ? 4 : 2], masks)));
      if (g2 && ov) {  // join
        hipEventRecord(c->sev[5], c->side[0]);
        c->cur = nullptr;
        hipStreamWaitEvent(c->stream, c->sev[5], 0);
      }
      return GS_OK;
    };
    // A host-pointer call runs the G2 side FIRST: every output but the last proof element crosses PCIe under later
    // kernels (the commitments of a side under its variable-base kernel, the first side's proof element under the second
    // side), and the one that is left after the last kernel is then theta (1/8 of the output bytes) rather than pi.
    const bool g2_first = c->pipe && !ov && N >= 16 * c->simd_slots;
    if (!g2_first) RC(side((F1*)nullptr));
    RC(side((F2*)nullptr));
    if (g2_first) RC(side((F1*)nullptr));
    return GS_OK;
  }

  // rerandomization of commitments and proofs without the witness, for all four types:
  //   c' = c + R' U_x,  d' = d + S' V_y,
  //   pi'    = pi + R'^T iota2(B) + (R'^T Gamma) d + (R'^T Gamma S' - T'^T) V_y
  //   theta' = theta + S'^T iota1(A) + (S'^T Gamma^T) c + T' U_x          (c, d: the OLD commitments)
  // The scalars are the prover's own with no witness scalars: k_prep_prove with xs = ys = NULL computes
  // Psi' = R'^T Gamma, Phi' = S'^T Gamma^T, Omega' = Psi' S' - T'^T, rho' = R'^T b, sigma' = S'^T a.
  // shared: a Statement -- ONE copy of c, d, R', S' (stride 0) for all N equations; the commitments are updated once.
  static int rerandomize(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G,
                         const void* xc, const void* yc, const void* pi, const void* th, const void* R, const void* Sm,
                         const void* T, void* xco, void* yco, void* pio, void* tho, bool shared) {
    const Shape sh(ty, m, n);
    PoolMap pm = prove_pool(m, n, sh.kx, sh.ky);
    void* pool;
    RC(scratch(c, "rerand.pool", N * pm.total * sizeof(S), &pool));
    RangeGuard rg_all("gs.rerandomize");
    RC(need(c, BIT(RI_G) | BIT(RI_R) | BIT(RI_S) | BIT(RI_T) | (sh.xg ? 0u : BIT(RI_A)) | (sh.yg ? 0u : BIT(RI_B))));
    RC(prep_prove(c, "k_prep_rerand", N, m, n, sh.kx, sh.ky, G, R, Sm, T, nullptr, nullptr, sh.xg ? nullptr : A,
                  sh.yg ? nullptr : B, pm, pool, shared));
    // one side over NN equations: the commitments (coms) and / or the proof elements (proofs) of that side
    auto side = [&](auto* ftag, size_t NN, bool coms, bool proofs, const char* tag) -> int {
      typedef std::remove_pointer_t<decltype(ftag)> F;
      constexpr bool g2 = std::is_same<F, F2>::value;
      const bool grp = g2 ? sh.yg : sh.xg;
      const int nv = g2 ? n : m, nc = g2 ? m : n, kc = g2 ? sh.ky : sh.kx, npf = g2 ? sh.kx : sh.ky,
                np = proofs ? npf : 0;
      const uint32_t zp = (uint32_t)(g2 ? Z::G2 : Z::G1);
      SidePlan sp;
      sp.tm = np ? pick_tm(c, fillN(c, NN), grp ? nv + nc : nv, 2 * np, g2, np) : 1;
      if (g2)
        build_rerand_side(sp, coms, nv, nc, grp, kc, np, pm.SC, pm.RC, pm.PSI, pm.OM, pm.RHO);
      else
        build_rerand_side(sp, coms, nv, nc, grp, kc, np, pm.RC, pm.SC, pm.PHI, pm.TC, pm.SIG);
      const ArrTab arrs = arr_tab({{0, g2 ? yc : xc, shared ? 0u : (uint32_t)nv * 2 * zp},
                                   {1, g2 ? B : A, (uint32_t)nc * zp, grp},
                                   {2, g2 ? pi : th, (uint32_t)npf * 2 * zp}});
      const OutTab outs = out_tab(g2 ? yco : xco, (uint32_t)nv * 2 * zp, g2 ? pio : tho, (uint32_t)npf * 2 * zp);
      RangeGuard rg(g2 ? "gs.rerandomize.g2" : "gs.rerandomize.g1");
      const unsigned in_com = BIT(g2 ? RI_YC : RI_XC), in_pf = BIT(g2 ? RI_PI : RI_TH), in_k = BIT(g2 ? RI_B : RI_A);
      const unsigned masks[4] = {in_com | (proofs ? in_pf : 0u), proofs ? in_k : 0u, coms ? BIT(g2 ? RO_YC : RO_XC) : 0u,
                                 proofs ? BIT(g2 ? RO_PI : RO_TH) : 0u};
      const void* tab = g2 ? c->tabs->tab16_g2.p : c->tabs->tab16_g1.p;
      return run_side<C, F>(c, tag, NN, sp, arrs, (const S*)pool, pm.total, (const Aff<F>*)tab, outs, nullptr, nullptr,
                            nullptr, masks);
    };
    if (shared) {  // the Statement's commitments once (equation 0 of the pool holds R', S'), then the E proofs
      RC(side((F1*)nullptr, 1, true, false, ".rc1"));
      RC(side((F2*)nullptr, 1, true, false, ".rc2"));
      RC(side((F1*)nullptr, N, false, true, ".rg1"));
      return side((F2*)nullptr, N, false, true, ".rg2");
    }
    // (host-pointer calls: the G2 side first, as in prove -- theta is then the last output to cross PCIe)
    if (c->pipe && N >= 16 * c->simd_slots) {
      RC(side((F2*)nullptr, N, true, true, ".rg2"));
      return side((F1*)nullptr, N, true, true, ".rg1");
    }
    RC(side((F1*)nullptr, N, true, true, ".rg1"));
    return side((F2*)nullptr, N, true, true, ".rg2");
  }

  // simulation with the hiding CRS's trapdoor (t1, t2: W1 = t1 u0, W2 = t2 v0), MSMEG1 / MSMEG2 / QuadEqu, no witness:
  //   c_i = sum_a Rc_ia u_a,  d_j = sum_b Sc_jb v_b                      (commitments to nothing in particular)
  //   QuadEqu: theta = Tf u0, pi = OM v0
  //   MSMEG1:  pi_k = Tf[0][k] v0,  theta = (O, V) + OM_0 u0 + OM_1 u1,  V = sum_j Sc_j A_j - t2 T
  //   MSMEG2:  theta_l = Tf[l][0] u0,  pi = (O, V) + OM_0 v0 + OM_1 v1,  V = sum_i Rc_i B_i - t1 T
  // (OM: k_prep_sim).  Every output component is one k_fix lane; V is n + 1 (m + 1) variable-base terms behind the
  // fixed-base lane of component 1.  The pool holds -t and products with t: it is zeroed behind its last reader.
  // shared: a Statement -- ONE copy of Rc, Sc (stride 0); the commitments are written once, then the N proofs.
  static int simulate(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G,
                      const void* tg, const void* Rc, const void* Sc, const void* Tf, void* xcoms, void* ycoms,
                      void* pi, void* theta, bool shared) {
    const Shape sh(ty, m, n);
    const PoolMap pm = pool_layout({{&PoolMap::RC, m * sh.kx}, {&PoolMap::SC, n * sh.ky}, {&PoolMap::TC, sh.ky * sh.kx},
                                    {&PoolMap::OM, 2}, {&PoolMap::NT, 1}});
    void* pool;
    const size_t pool_bytes = N * pm.total * sizeof(S);
    RC(scratch(c, "sim.pool", pool_bytes, &pool));
    struct PoolWipe {  // whatever happens below: on the stream, after the kernels enqueued so far
      gs_ctx* c;
      void* p;
      size_t bytes;
      ~PoolWipe() { hipMemsetAsync(p, 0, bytes, c->stream); }
    } wipe{c, pool, pool_bytes};
    RangeGuard rg_all("gs.simulate");
    RC(need(c, BIT(SI_G) | BIT(SI_R) | BIT(SI_S) | BIT(SI_T) | (sh.xg ? 0u : BIT(SI_A)) | (sh.yg ? 0u : BIT(SI_B)) |
                   (ty == GS_QUAD ? BIT(SI_TG) : 0u)));
    RC(launch_seg<k_prep_sim<C>>(c, "k_prep_sim", N, 64, N, ty, m, n, (const S*)G, sh.xg ? (const S*)nullptr : (const S*)A,
                                 sh.yg ? (const S*)nullptr : (const S*)B, ty == GS_QUAD ? (const S*)tg : (const S*)nullptr,
                                 (const S*)Rc, (const S*)Sc, (const S*)Tf, (const S*)c->skey.p, pm, (S*)pool,
                                 shared ? 1 : 0));
    // one side over NN equations: the commitments (coms non-null) and / or the proof elements of that side
    auto side = [&](auto* ftag, size_t NN, void* coms, bool proofs, const char* tag) -> int {
      typedef std::remove_pointer_t<decltype(ftag)> F;
      constexpr bool g2 = std::is_same<F, F2>::value;
      const bool grp = g2 ? sh.yg : sh.xg;  // a group-valued side carries V
      const int nv = g2 ? n : m, nc = g2 ? m : n, npf = g2 ? sh.kx : sh.ky, rc = g2 ? pm.SC : pm.RC,
                cs = g2 ? pm.RC : pm.SC;
      const uint32_t zp = (uint32_t)(g2 ? Z::G2 : Z::G1);
      SidePlan sp;
      sp.tm = proofs && grp ? pick_tm(c, fillN(c, NN), nc + 1, 1, g2, 1) : 1;
      ComOutputs out{sp};
      if (coms) {
        out.add(nv, 0, 0, [&](int i, int k, ComOutputs& o) {
          if (grp)
            o.fix(rc + 2 * i, tb_u(0, k), rc + 2 * i + 1, tb_u(1, k), 0xFF, 0);
          else
            o.fix(rc + i, tb_u(0, k), 0, 0xFF, 0xFF, 0);
        });
        sp.ncom = nv;
      }
      if (proofs)
        out.add(npf, 1, 0, [&](int l, int k, ComOutputs& o) {
          if (!grp)  // a multiple of u0 / v0: Tf, or QuadEqu's pi'
            return o.fix(g2 && ty == GS_QUAD ? pm.OM : pm.TC + l, tb_u(0, k), 0, 0xFF, 0xFF, 0);
          o.fix(pm.OM, tb_u(0, k), pm.OM + 1, tb_u(1, k), 0xFF, 0);
          if (k == 0) return;  // (O, V)
          std::vector<VarTask> terms;
          for (int j = 0; j < nc; j++) terms.push_back(mkvar(cs + j, 1, j, 0));
          terms.push_back(mkvar(pm.NT, 2, 0, 0));
          o.terms(terms);
        });
      const ArrTab arrs = arr_tab({{1, g2 ? B : A, (uint32_t)nc * zp, grp}, {2, tg, zp, grp}});
      const OutTab outs = out_tab(coms, (uint32_t)nv * 2 * zp, g2 ? pi : theta, (uint32_t)npf * 2 * zp);
      RangeGuard rg(g2 ? "gs.simulate.g2" : "gs.simulate.g1");
      const unsigned masks[4] = {0u, proofs && grp ? BIT(g2 ? SI_B : SI_A) | BIT(SI_TG) : 0u,
                                 coms ? BIT(g2 ? SO_YC : SO_XC) : 0u, proofs ? BIT(g2 ? SO_PI : SO_TH) : 0u};
      const void* tab = g2 ? c->tabs->tab16_g2.p : c->tabs->tab16_g1.p;
      return run_side<C, F>(c, tag, NN, sp, arrs, (const S*)pool, pm.total, (const Aff<F>*)tab, outs, nullptr, nullptr,
                            nullptr, masks);
    };
    if (shared) {  // the Statement's commitments once (equation 0 of the pool holds Rc, Sc), then the E proofs
      if (xcoms) RC(side((F1*)nullptr, 1, xcoms, false, ".sc1"));
      if (ycoms) RC(side((F2*)nullptr, 1, ycoms, false, ".sc2"));
      xcoms = ycoms = nullptr;
    }
    RC(side((F1*)nullptr, N, xcoms, true, ".sm1"));
    return side((F2*)nullptr, N, ycoms, true, ".sm2");
  }

  // commitments only (commit.rs:59-256): a "prove" side with no proof elements
  template <class F>
  static int commit(gs_ctx* c, size_t count, bool group, const void* vars, const void* rand, void* out,
                    const Aff<F>* tab, const char* tag) {
    int kc = group ? 2 : 1;
    const size_t bsz = sizeof(Aff<F>) == sizeof(A1) ? Z::G1 : Z::G2;  // boundary bytes of one point
    const PoolMap pm = pool_layout({{&PoolMap::RC, kc}, {&PoolMap::XC, 1}});
    void* pool;
    RC(scratch(c, "commit.pool", count * pm.total * sizeof(S), &pool));
    // reuse k_prep_prove with m = 1 variable per "equation", no Gamma work (n = 0, ky = 0)
    RC(launch_seg<k_prep_prove<C>>(c, "k_prep_commit", count, 64, count, 1, 0, kc, 0, (const S*)nullptr, (const S*)rand,
              (const S*)nullptr, (const S*)nullptr, group ? nullptr : (const S*)vars, (const S*)nullptr,
              (const S*)nullptr, (const S*)nullptr, pm, (S*)pool, 0));
    SidePlan sp;
    build_side(sp, true, 1, 0, group, kc, 0, pm.RC, pm.XC, 0, 0, 0, 0);
    const ArrTab arrs = arr_tab({{0, vars, (uint32_t)bsz, group}});
    const OutTab outs = out_tab(out, (uint32_t)(2 * bsz));
    return run_side<C, F>(c, tag, count, sp, arrs, (const S*)pool, pm.total, tab, outs);
  }

  // --------------------------------------------------------------- verify --
  struct VerifyPlan {
    SidePlan g1;                      // PA_j (j<n) [+ PB] as Com1-shaped pairs
    std::vector<MillerTask> mt;
    CellMap cm;
    int npa;                          // Com1 elements in the PA scratch per equation
  };

  static void build_verify_g1(VerifyPlan& vp, const Shape& s, const PoolMap& pm, int tm) {
    const int m = s.m, n = s.n;
    // ---- G1-side points: PA_j.a = map_a_j.a + sum_i Gamma_ij c_i.a ;  PB.a = sum_i b_i c_i.a - lin_t
    // engine arrays: 0 = xcoms as 2m G1 points, 1 = A (group), 2 = target (MSMEG1)
    SidePlan& sp = vp.g1;
    sp.tm = tm;
    if (tm < 0) {  // shared per-base tables: groups of 8 terms, array 0 = the 2 m components of the X commitments
      sp.tm = 8;
      sp.tab_bases = 2 * m;
    }
    ComOutputs out{sp};
    out.add(n, 0, 0, [&](int j, int a, ComOutputs& o) {
      if (!s.xg)
        o.fix(pm.AC + j, tb_w(a), 0, 0xFF, 0xFF, 0);
      else if (a == 1)
        o.fix(0, 0xFF, 0, 0xFF, 1, j);
      std::vector<VarTask> terms;
      com_terms(terms, pm.GC + j, n, m, 0, a);
      o.terms(terms);
    });
    vp.npa = n;
    if (!s.yg) {
      out.add(1, 0, n, [&](int, int a, ComOutputs& o) {
        std::vector<VarTask> terms;
        com_terms(terms, pm.BC, 1, m, 0, a);
        o.terms(terms);
        if (s.ty == GS_MSMEG1 && a == 1) o.fix(0, 0xFF, 0, 0xFF, 2, 0, 1);  // - t
        if (s.ty == GS_QUAD) o.fix(pm.NT, tb_w(a), 0, 0xFF, 0xFF, 0);       // (-t) W1.a
      });
      vp.npa = n + 1;
    }
  }
  // P arrays: 0 PA scratch, 1 xcoms, 2 crs G1 consts, 3 theta
  // Q arrays: 0 ycoms, 1 B, 2 crs G2 consts, 3 pi, 4 target (MSMEG2)
  static void build_verify_miller(VerifyPlan& vp, int curve, const Shape& s, double budget, bool twin, bool lt) {
    // ---- Miller tasks.  Pairs of cell (a, b): G1 argument = component a, G2 argument = component b.
    //  twin  : one task list per b, each lane takes `ch` (Q, P0, P1) triples and keeps two accumulators
    //          (lines of Q computed once) -- less total work, pays off once the chip is full;
    //  single: one task list per cell, `ch` (P, Q) pairs and one accumulator per lane -- more, shorter lanes.
    vp.mt.clear();
    for (int cell = 0; cell < (twin ? 2 : 4); cell++) {
      int b = twin ? cell : (cell & 1), a = twin ? 0 : (cell >> 1);
      std::vector<PairRef> pr;
      add_pairs(pr,
                {{{0, 0}, {0, 0}, s.n, 0},                          // (PA_j, d_j)
                 {{1, 0}, {1, 0, false}, s.yg ? s.m : 0, 0},        // (c_i, B_i)
                 {{0, s.n}, {2, 2}, s.yg ? 0 : 1, 0},               // (PB, W2)
                 {{2, 0}, {3, 0}, s.kx, 1},                         // (-u_k, pi_k)
                 {{3, 0}, {2, 0}, s.ky, 1},                         // (-theta_l, v_l)
                 {{2, 2}, {4, 0, false}, s.ty == GS_MSMEG2, 1}},    // (-W1, t)
                a, b);
      int lo = (int)vp.mt.size();
      chunk_tasks(vp.mt, pr, budget, b, !twin, mcost(curve, twin), lt);
      int hi = (int)vp.mt.size();
      if (twin) {
        for (int aa = 0; aa < 2; aa++) {
          vp.cm.lo[2 * aa + b] = lo;
          vp.cm.hi[2 * aa + b] = hi;
          vp.cm.sub[2 * aa + b] = aa;
        }
      } else {
        vp.cm.lo[cell] = lo;
        vp.cm.hi[cell] = hi;
        vp.cm.sub[cell] = 0;
      }
    }
  }

  // Gamma as k_prep_verify[_rlc] takes it.  Large arities bring it to canonical form in the pool first, one lane per
  // entry, and the preparation kernel then leaves it alone (*g = null).
  static int prep_gamma(gs_ctx* c, size_t N, int m, int n, const void* G, const PoolMap& pm, void* pool, const S** g) {
    const bool wide = wide_prep(m, n);
    *g = wide ? nullptr : (const S*)G;
    if (!wide) return GS_OK;
    return launch_seg<k_fr_canonical<C>>(c, "k_fr_canonical", N * (size_t)m * n, 64, N * (size_t)m * n, m * n, (const S*)G,
              pm.total, (S*)pool + pm.GC);
  }
  // the line tables a Miller launch reads (null: every line is stepped)
  static const Line<C>* lines(const gs_ctx* c) { return (const Line<C>*)(c->line_tables ? c->tabs->line_tab.p : nullptr); }
  // Miller tail of the two RLC verifiers: the single-accumulator task list `mt` (plan_miller_single) goes up as `tag`.mt
  // and runs as k_miller.`tag` into the scratch `tag`.mpart (mt.size() partials per equation).
  // (ostride 2 leaves the partials in the layout k_cell_fold reads: slot 0 of a pair)
  static int miller_single(gs_ctx* c, const std::string& tag, size_t N, const std::vector<MillerTask>& mt,
                           const ArrTab& parr, const ArrTab& qarr, void** mpart, int ostride = 1) {
    const MillerTask* dmt;
    RC(upload(c, (tag + ".mt").c_str(), mt, &dmt));
    const int ntask = (int)mt.size();
    RC(scratch(c, (tag + ".mpart").c_str(), N * ntask * ostride * sizeof(GT), mpart));
    miller_work_hint(c, N, mt, false);
    return launch_seg<k_miller<C, false>>(c, ("k_miller." + tag).c_str(), N * ntask, 64, N * ntask, ntask, dmt, parr, qarr,
              (GT*)*mpart, ostride, lines(c));
  }

  // Q arrays of the exact verifier and of rlc_front: 0 ycoms, 1 B, 2 crs G2 consts, 3 pi, 4 target (MSMEG2)
  // (shared: a Statement's equations share the commitments)
  static ArrTab q_arrays(const gs_ctx* c, const VerifyIn& v, bool shared) {
    return arr_tab({{0, v.ycoms, shared ? 0u : (uint32_t)(v.sh.n * Z::COM2)},
                    {1, v.B, (uint32_t)(v.sh.m * Z::G2)},
                    {2, c->tabs->crs_g2.p, 0},
                    {3, v.pi, (uint32_t)(v.sh.kx * Z::COM2)},
                    {4, v.target, (uint32_t)Z::G2}});
  }

  // shared front of both verifier modes: G1-side points + Miller partials
  static int verify_front(gs_ctx* c, const VerifyIn& v, VerifyPlan& vp, void** mpart_out, bool shared) {
    const Shape& s = v.sh;
    const int ty = s.ty, m = s.m, n = s.n;
    const size_t N = v.N;
    const PoolMap pm = pool_layout({{&PoolMap::GC, m * n}, {&PoolMap::AC, n}, {&PoolMap::BC, m}, {&PoolMap::NT, 1}});
    void* pool;
    RC(scratch(c, "verify.pool", N * pm.total * sizeof(S), &pool));
    RC(need(c, BIT(VI_G) | (s.xg ? 0u : BIT(VI_A)) | (s.yg ? 0u : BIT(VI_B)) | (ty == GS_QUAD ? BIT(VI_TG) : 0u)));
    const S* g;
    RC(prep_gamma(c, N, m, n, v.G, pm, pool, &g));
    RC(launch_seg<k_prep_verify<C>>(c, "k_prep_verify", N, 64, N, m, n, g, s.xg ? nullptr : (const S*)v.A,
              s.yg ? nullptr : (const S*)v.B, ty == GS_QUAD ? (const S*)v.target : nullptr, pm, (S*)pool));
    // lane shape for this batch size: single or twin accumulators (the twin task list on one lane with two
    // accumulators, or on a pair of lanes with one each), lane-cost budget (cost model above)
    int mode = 0;  // 0 single, 1 twin, 2 pair (LDS exchange), 3 pair (DPP exchange)
    double budget = 3 * 4621.0;
    {
      // the choice depends on the shape, the batch size and the overrides only: remembered per context
      char key[96];
      const size_t NF = fillN(c, N);
      snprintf(key, sizeof key, "%d.%d.%d.%zu.%d.%d.%d", ty, m, n, NF, c->miller_twin, c->miller_ch, (int)c->line_tables);
      auto hit = c->miller_choice.find(key);
      if (hit != c->miller_choice.end()) {
        mode = hit->second.first;
        budget = hit->second.second;
      } else {
        double best = -1;
        for (int md = 0; md < 3; md++) {
          if (c->miller_twin >= 0 && md != (c->miller_twin == 3 ? 2 : c->miller_twin)) continue;
          if (c->miller_twin < 0 && md == 2 && !GS_PLAN_PAIR) continue;
          for (double cand : miller_budgets(c, md != 0)) {
            VerifyPlan tmp;
            build_verify_miller(tmp, c->curve, s, cand, md != 0, c->line_tables);
            double cost = miller_cost(c, NF, tmp.mt, md != 0, md == 2);
            if (md == 2) cost *= 0.97;  // measured: the same triples finish 3-4 % sooner with one accumulator per lane
            if (best < 0 || cost < best) {
              best = cost;
              mode = md;
              budget = cand;
            }
          }
        }
        // planned exchange of the pair kernel: LDS slots on BLS12-381, DPP on BN254.  (DPP won until the round loop's
        // products moved into one lambda, 166.7 vs 170.0 ms; with that shape the partner's line parked in LDS across
        // the lane's own product beats the 84 registers it occupies: 147.6 vs 155.0 ms at 2^16, 41.3 vs 42.5 at 2^14,
        // 12.7 vs 13.2 at 2^12; BN254's shorter lines keep DPP ahead by 0.6 %: profiles/r3/ab_exchange.txt)
        if (mode == 2) mode = c->miller_twin == 3 ? 3 : c->miller_twin == 2 ? 2 : (c->curve == 0 ? 2 : 3);
        if (c->miller_choice.size() > 4096) c->miller_choice.clear();
        c->miller_choice[key] = std::make_pair(mode, budget);
      }
    }
    const bool twin = mode != 0;
    // the Gamma^T c lanes: Straus groups with their own tables, or (large arities: every base serves 2 n outputs)
    // lanes over shared per-base window tables -- measured in profiles/r3/large_arity_334.json
    // (planned only while the tables -- N x 2 m bases x 128 entries, affine + Jacobian staging -- stay below 8 GB)
    const double tab8_bytes = (double)N * 2.0 * m * 128.0 * (double)(sizeof(A1) + sizeof(Jac<F1>));
    // (the shared base tables are read by endomorphism-decomposed lanes: not with "endo" off)
    const bool tab8 = c->endo && (c->var_tab == 1 || (c->var_tab < 0 && wide_prep(m, n) && n >= 32 && tab8_bytes <= 8e9));
    build_verify_g1(vp, s, pm, tab8 ? -1 : pick_tm(c, fillN(c, N), m, 2 * n, false, n));
    build_verify_miller(vp, c->curve, s, budget, twin, c->line_tables);
    // G1-side points
    void* pa;
    RC(scratch(c, "verify.pa", N * vp.npa * Z::COM1, &pa));
    {
      // (a Statement's equations share the commitments)
      const ArrTab arrs = arr_tab({{0, v.xcoms, shared ? 0u : (uint32_t)(m * Z::COM1)},
                                   {1, v.A, (uint32_t)(n * Z::G1), s.xg},
                                   {2, v.target, (uint32_t)Z::G1, ty == GS_MSMEG1}});
      const OutTab outs = out_tab(pa, (uint32_t)(vp.npa * Z::COM1));
      RangeGuard rg("gs.verify.g1");
      RC(need(c, BIT(VI_XC) | BIT(VI_A) | BIT(VI_TG) * (ty == GS_MSMEG1 ? 1u : 0u)));
      RC((run_side<C, F1>(c, ".vg1", N, vp.g1, arrs, (const S*)pool, pm.total, (const A1*)c->tabs->tab16_g1.p, outs)));
    }
    // Miller
    RangeGuard rg_m("gs.verify.miller");
    RC(need(c, 0xFFu));  // every input array from here on
    const MillerTask* dmt;
    RC(upload(c, "verify.mt", vp.mt, &dmt));
    int ntask = (int)vp.mt.size();
    void* mpart;
    RC(scratch(c, "verify.mpart", 2 * N * ntask * sizeof(GT), &mpart));
    const ArrTab parr = arr_tab({{0, pa, (uint32_t)(vp.npa * Z::COM1)},
                                 {1, v.xcoms, shared ? 0u : (uint32_t)(m * Z::COM1)},
                                 {2, c->tabs->crs_g1.p, 0},
                                 {3, v.theta, (uint32_t)(s.ky * Z::COM1)}});
    const ArrTab qarr = q_arrays(c, v, shared);
    miller_work_hint(c, N, vp.mt, twin);
    if (getenv("GS_PLAN_TRACE")) {
      const MCost mc = mcost(c->curve, twin);
      fprintf(stderr, "[plan] verify ty %d N %zu (fill %zu) m %d n %d: miller mode %d budget %.0f, %d tasks, lanes:", ty, N,
              fillN(c, N), m, n, mode, budget, (int)ntask);
      for (const MillerTask& t : vp.mt) {
        double l = mc.base;
        for (int q = 0; q < t.np; q++) l += pair_fixed(c->line_tables, t.pr[q]) ? mc.fix : mc.var;
        fprintf(stderr, " %.0f", mode >= 2 ? pair_lane_cost(c, t) : l);
      }
      fprintf(stderr, "; waves %zu\n", ((mode >= 2 ? 2 : 1) * N * ntask + 63) / 64);
    }
    if (mode == 2)
      RC(launch_seg<k_miller_pair<C, false>>(c, "k_miller.pair", 2 * N * ntask, 64, 2 * N * ntask, ntask, dmt, parr, qarr,
                (GT*)mpart, lines(c)));
    else if (mode == 3)
      RC(launch_seg<k_miller_pair<C, true>>(c, "k_miller.pairdpp", 2 * N * ntask, 64, 2 * N * ntask, ntask, dmt, parr, qarr,
                (GT*)mpart, lines(c)));
    else if (twin)
      RC(launch_seg<k_miller<C, true>>(c, "k_miller.twin", N * ntask, 64, N * ntask, ntask, dmt, parr, qarr, (GT*)mpart, 2,
                lines(c)));
    else
      RC(launch_seg<k_miller<C, false>>(c, "k_miller", N * ntask, 64, N * ntask, ntask, dmt, parr, qarr, (GT*)mpart, 2,
                lines(c)));
    *mpart_out = mpart;
    return GS_OK;
  }

  static int verify(gs_ctx* c, const VerifyIn& v, uint8_t* ok, bool shared) {
    const size_t N = v.N;
    const uint8_t* target = v.sh.ty == GS_PPE ? (const uint8_t*)v.target : nullptr;
    VerifyPlan vp;
    void* mpart;
    RangeGuard rg_all("gs.verify");
    RC(verify_front(c, v, vp, &mpart, shared));
    RangeGuard rg_f("gs.verify.final");
    int ntask = (int)vp.mt.size();
    // large arities: hundreds of Miller partials per cell -- fold runs of K in parallel until k_final's own serial
    // product is short (segmented K-ary tree in GT)
    CellMap cm = vp.cm;
    {
      const int K = 8;
      for (int level = 0;; level++) {
        int longest = 0;
        for (int q = 0; q < 4; q++) longest = std::max(longest, cm.hi[q] - cm.lo[q]);
        if (longest <= 2 * K) break;
        CellMap out;
        int nt_out = 0, runs_max = (longest + K - 1) / K;
        for (int q = 0; q < 4; q++) {
          out.lo[q] = nt_out;
          nt_out += (cm.hi[q] - cm.lo[q] + K - 1) / K;
          out.hi[q] = nt_out;
          out.sub[q] = 0;
        }
        void* folded;
        RC(scratch(c, level & 1 ? "verify.mfold1" : "verify.mfold0", 2 * N * (size_t)nt_out * sizeof(GT), &folded));
        size_t total = N * 4 * (size_t)runs_max;
        RC(launch_seg<k_cell_fold<C>>(c, "k_cell_fold", total, 64, total, runs_max, ntask, cm, (const GT*)mpart, K, nt_out, out,
                  (GT*)folded));
        mpart = folded;
        ntask = nt_out;
        cm = out;
      }
    }
    void* cellok;
    RC(scratch(c, "verify.cellok", N * 4, &cellok));
    if (coop_lanes(c, fillN(c, N) * 4))
      RC(launch_seg<k_final_coop<C>>(c, "k_final.coop", (N * 4 + 20) / 21 * 63, 63, N, ntask, cm, (const GT*)mpart, target,
                (uint8_t*)cellok));
    else
      RC(launch_seg<k_final<C>>(c, "k_final", N * 4, 64, N, ntask, cm, (const GT*)mpart, target, (uint8_t*)cellok));
    RC(launch_seg<k_and4>(c, "k_and4", N, 64, N, (const uint8_t*)cellok, ok));
    return GS_OK;
  }

  // ------------------------------------------------------------- evaluate --
  // The left-hand side of an equation at a witness (statement.rs:17-21), written to `out` -- or, with out null, compared
  // with `target` into ok[N] (gs_check_witness_*).  No CRS element is read.
  //   PPE      W_j = A_j + sum_i Gamma_ij X_i: n outputs over the SAME m bases (share_tables; the shared window tables at
  //            large arity), A_j the affine addend of a table-less k_fix lane; then prod_j e(W_j, Y_j) prod_i e(X_i, B_i):
  //            m + n stepped pairs, one accumulator and one final exponentiation per equation
  //   MSMEG1/2 ONE output over m + n variable-base terms, the Gamma term folded into their scalars by k_prep_eval
  //   QuadEqu  k_prep_eval alone
  // shared: a Statement -- ONE copy of X, Y (stride 0) for all N equations.
  // One MSME output.  G1: array 0 = X (scalars c_i at BC), 1 = A (y_j at YC); G2: array 0 = Y (d_j at AC), 1 = B (x_i at XC)
  template <class F>
  static int eval_msme(gs_ctx* c, const Shape& sh, size_t N, const PoolMap& pm, const void* pool, const void* V,
                       const void* K, const void* target, void* out, uint8_t* ok, bool shared) {
    constexpr bool g2 = std::is_same<F, F2>::value;
    const uint32_t zp = (uint32_t)(g2 ? Z::G2 : Z::G1);
    const int nv = g2 ? sh.n : sh.m, nc = g2 ? sh.m : sh.n, sv = g2 ? pm.AC : pm.BC, sc = g2 ? pm.XC : pm.YC;
    SidePlan sp;
    sp.points = true;
    sp.tm = pick_tm(c, fillN(c, N), nv + nc, 1, g2, 1);
    std::vector<VarTask> terms;
    for (int i = 0; i < nv; i++) terms.push_back(mkvar(sv + i, 0, i, 0));
    for (int j = 0; j < nc; j++) terms.push_back(mkvar(sc + j, 1, j, 0));
    int slot = 0;
    add_var_terms(sp, terms, slot);
    sp.red.push_back(mkred(0, slot, 0, 0, 0, 0));
    sp.nslots = slot;
    void* val = out;
    if (!out) RC(scratch(c, "eval.val", N * zp, &val));
    const ArrTab arrs = arr_tab({{0, V, shared ? 0u : (uint32_t)nv * zp}, {1, K, (uint32_t)nc * zp}});
    const OutTab outs = out_tab(val, zp);
    RangeGuard rg(g2 ? "gs.eval.g2" : "gs.eval.g1");
    const unsigned masks[4] = {0u, BIT(g2 ? EI_Y : EI_X) | BIT(g2 ? EI_B : EI_A), 0u, out ? BIT(EO_T) : 0u};
    const void* tab = g2 ? c->tabs->tab16_g2.p : c->tabs->tab16_g1.p;  // (no fixed-base lane: never read)
    RC((run_side<C, F>(c, g2 ? ".ev2" : ".ev1", N, sp, arrs, (const S*)pool, pm.total, (const Aff<F>*)tab, outs, nullptr,
                       nullptr, nullptr, masks)));
    if (out) return GS_OK;
    RC(need(c, BIT(EI_TG)));
    return launch_seg<k_eval_cmp>(c, "k_eval_cmp", N, 64, N, (int)(zp / 4), (const uint32_t*)val, (const uint32_t*)target, ok);
  }
  static int eval(gs_ctx* c, int ty, size_t N, int m, int n, const void* X, const void* Y, const void* A, const void* B,
                  const void* G, const void* target, void* out, uint8_t* ok, bool shared) {
    const Shape sh(ty, m, n);
    const bool wide = wide_prep(m, n), check = out == nullptr;
    const int sv = shared ? 1 : 0;
    RangeGuard rg_all("gs.eval");
    const PoolMap pm = ty == GS_PPE      ? pool_layout({{&PoolMap::GC, m * n}})
                       : ty == GS_MSMEG1 ? pool_layout({{&PoolMap::YC, n}, {&PoolMap::BC, m}})
                       : ty == GS_MSMEG2 ? pool_layout({{&PoolMap::XC, m}, {&PoolMap::AC, n}})
                                         : pool_layout({{&PoolMap::BC, m}});
    void* pool;
    RC(scratch(c, "eval.pool", N * pm.total * sizeof(S), &pool));
    const S *xs = sh.xg ? nullptr : (const S*)X, *ys = sh.yg ? nullptr : (const S*)Y;
    const S *as = sh.xg ? nullptr : (const S*)A, *bs = sh.yg ? nullptr : (const S*)B;
    // (host-pointer calls: the scalars first; group-valued arrays are not read before their side)
    RC(need(c, BIT(EI_G) | (sh.xg ? 0u : BIT(EI_X) | BIT(EI_A)) | (sh.yg ? 0u : BIT(EI_Y) | BIT(EI_B)) |
                   (ty == GS_QUAD && check ? BIT(EI_TG) : 0u)));
    if (ty == GS_PPE) {
      const S* g;
      RC(prep_gamma(c, N, m, n, G, pm, pool, &g));
      if (g)
        RC(launch_seg<k_prep_eval<C>>(c, "k_prep_eval", N, 64, N, ty, m, n, g, xs, ys, as, bs, pm, (S*)pool, sv, 0,
                  (const S*)nullptr, (S*)nullptr, (uint8_t*)nullptr));
    } else {
      if (wide) {  // one lane per output scalar
        const int W = ty == GS_QUAD ? m : m + n;
        RC(launch_seg<k_prep_eval_wide<C>>(c, "k_prep_eval.a", N * (size_t)W, 64, N * (size_t)W, W, ty, m, n, (const S*)G,
                  xs, ys, as, bs, pm, (S*)pool, sv));
      }
      if (!wide || ty == GS_QUAD)
        RC(launch_seg<k_prep_eval<C>>(c, "k_prep_eval", N, 64, N, ty, m, n, (const S*)G, xs, ys, as, bs, pm, (S*)pool, sv,
                  wide ? 1 : 0, check ? (const S*)target : (const S*)nullptr, check ? (S*)nullptr : (S*)out,
                  check ? ok : (uint8_t*)nullptr));
    }
    if (ty == GS_QUAD) return GS_OK;
    if (ty == GS_MSMEG1) return eval_msme<F1>(c, sh, N, pm, pool, X, A, target, out, ok, shared);
    if (ty == GS_MSMEG2) return eval_msme<F2>(c, sh, N, pm, pool, Y, B, target, out, ok, shared);
    // ---- PPE: W_j, arrays 0 = X, 1 = A.  Shared per-base window tables as in the verifier's Gamma^T c (every base serves
    // n outputs): planned for large arities while the tables stay below 8 GB, never with "endo" off
    const double tab8_bytes = (double)N * m * 128.0 * (double)(sizeof(A1) + sizeof(Jac<F1>));
    const bool tab8 = c->endo && (c->var_tab == 1 || (c->var_tab < 0 && wide && n >= 32 && tab8_bytes <= 8e9));
    void* w;
    RC(scratch(c, "eval.w", N * n * Z::G1, &w));
    {
      SidePlan sp;
      sp.points = true;
      sp.tm = tab8 ? 8 : pick_tm(c, fillN(c, N), m, n, false, n);
      if (tab8) sp.tab_bases = m;
      int slot = 0;
      for (int j = 0; j < n; j++) {
        const int b = slot;
        sp.fix.push_back(mkfix(0, 0xFF, 0, 0xFF, 1, j, slot++));  // A_j
        std::vector<VarTask> terms;
        for (int i = 0; i < m; i++) terms.push_back(mkvar(pm.GC + i * n + j, 0, i, 0));
        add_var_terms(sp, terms, slot);
        sp.red.push_back(mkred(b, slot, b, b, 0, j));
      }
      sp.nslots = slot;
      const ArrTab arrs = arr_tab({{0, X, shared ? 0u : (uint32_t)(m * Z::G1)}, {1, A, (uint32_t)(n * Z::G1)}});
      const OutTab outs = out_tab(w, (uint32_t)(n * Z::G1));
      RangeGuard rg("gs.eval.g1");
      const unsigned masks[4] = {BIT(EI_A), BIT(EI_X), 0u, 0u};
      RC((run_side<C, F1>(c, ".ev1", N, sp, arrs, (const S*)pool, pm.total, (const A1*)c->tabs->tab16_g1.p, outs, nullptr,
                          nullptr, nullptr, masks)));
    }
    // ---- Miller: one accumulator per equation.  P arrays: 0 = W, 1 = X.  Q arrays: 0 = Y, 1 = B.  All lines stepped
    RangeGuard rg_m("gs.eval.miller");
    RC(need(c, BIT(EI_Y) | BIT(EI_B)));
    std::vector<PairRef> pr;
    for (int j = 0; j < n; j++) add_pair(pr, 0, j, 0, 0, j);  // (W_j, Y_j)
    for (int i = 0; i < m; i++) add_pair(pr, 1, i, 0, 1, i);  // (X_i, B_i)
    const ArrTab parr = arr_tab({{0, w, (uint32_t)(n * Z::G1)}, {1, X, shared ? 0u : (uint32_t)(m * Z::G1)}});
    const ArrTab qarr = arr_tab({{0, Y, shared ? 0u : (uint32_t)(n * Z::G2)}, {1, B, (uint32_t)(m * Z::G2)}});
    const std::vector<MillerTask> mt = plan_miller_single(c, fillN(c, N), pr);
    int ntask = (int)mt.size();
    // large arities: fold runs of K partials in parallel until the final lane's own serial product is short (as verify)
    const int K = 8;
    const int ostride = ntask > 2 * K ? 2 : 1;
    void* mpart;
    RC(miller_single(c, "eval", N, mt, parr, qarr, &mpart, ostride));
    for (int level = 0; ntask > 2 * K; level++) {
      CellMap cm, cmo;
      memset(&cm, 0, sizeof cm);
      memset(&cmo, 0, sizeof cmo);
      cm.hi[0] = ntask;
      const int nt_out = (ntask + K - 1) / K;
      cmo.hi[0] = nt_out;
      void* folded;
      RC(scratch(c, level & 1 ? "eval.mfold1" : "eval.mfold0", 2 * N * (size_t)nt_out * sizeof(GT), &folded));
      const size_t total = N * 4 * (size_t)nt_out;
      RC(launch_seg<k_cell_fold<C>>(c, "k_cell_fold", total, 64, total, nt_out, ntask, cm, (const GT*)mpart, K, nt_out, cmo,
                (GT*)folded));
      mpart = folded;
      ntask = nt_out;
    }
    RangeGuard rg_f("gs.eval.final");
    if (check) RC(need(c, BIT(EI_TG)));
    if (coop_lanes(c, fillN(c, N)))
      return launch_seg<k_final_eval_coop<C>>(c, "k_final_eval.coop", (N + 20) / 21 * 63, 63, N, ntask, ostride,
                (const GT*)mpart, (const uint8_t*)target, (uint8_t*)out, ok);
    return launch_seg<k_final_eval<C>>(c, "k_final_eval", N, 64, N, ntask, ostride, (const GT*)mpart,
              (const uint8_t*)target, (uint8_t*)out, ok);
  }

  // product of n internal-form GT elements at `buf` (clobbers buf/tmp); result exported in
  // boundary form to dst (one GT)
  static int gt_product(gs_ctx* c, size_t n, GT* buf, GT* tmp, uint8_t* dst) {
    const int K = 8;
    GT *in = buf, *out = tmp;
    while (n > 1) {
      size_t no = (n + K - 1) / K;
      RC(launch(c, "k_gt_prod", k_gt_prod<C>, no, 64, n, (const GT*)in, no, out, K));
      GT* t = in;
      in = out;
      out = t;
      n = no;
    }
    RC(launch(c, "k_gt_export", k_gt_export<C>, 1, 64, (size_t)1, (const GT*)in, dst));
    return GS_OK;
  }

  // Batched verifier.  acc[0] = prod_e prod_cells Miller(e,cell)^rho_{e,cell} (un-exponentiated),
  // acc[1] = prod_e t_e^rho_{e,11} (1 for non-PPE).  The exponents are FOLDED INTO THE G1 ARGUMENTS:
  //   prod_{a,b} e(P_a, Q_b)^{rho_ab} = prod_b e(rho_0b P_0 + rho_1b P_1, Q_b)
  // so every G2 argument is paired ONCE (20 instead of 40 pairs for the 4+4 PPE), there is one
  // accumulator per Miller lane, no per-cell exponentiation and one final exponentiation per batch.
  // Two passes of the linear-combination engine on G1:
  //   1. C'_ib = rho_0b c_i.0 + rho_1b c_i.1,  Th'_lb = rho_0b theta_l.0 + rho_1b theta_l.1
  //   2. P'_jb = rho_1b A_j + sum_i Gamma_ij C'_ib   (a_j rho_ab W1.a for scalar constants),
  //      PB'_b, U'_kb = rho_0b u_k.0 + rho_1b u_k.1, W1'_b      (Com-shaped: components b = 0, 1)
  // rlc_front: the pool, both G1 passes and the Miller launch; leaves N * ntask partials, equation-major, in rlc.mpart
  static int rlc_front(gs_ctx* c, const VerifyIn& v, const uint64_t* rho, void** mpart, int* ntask_out) {
    const Shape& s = v.sh;
    const int ty = s.ty, m = s.m, n = s.n;
    const size_t N = v.N;
    const PoolMap pm = pool_layout({{&PoolMap::GC, m * n}, {&PoolMap::BC, m}, {&PoolMap::RH, 4}, {&PoolMap::AR, 4 * n},
                                    {&PoolMap::NR, 4}});
    void* pool;
    RC(scratch(c, "rlc.pool", N * pm.total * sizeof(S), &pool));
    const S* g;
    RC(prep_gamma(c, N, m, n, v.G, pm, pool, &g));
    RC(launch(c, "k_prep_verify_rlc", k_prep_verify_rlc<C>, N, 64, N, m, n, g, s.xg ? nullptr : (const S*)v.A,
              s.yg ? nullptr : (const S*)v.B, ty == GS_QUAD ? (const S*)v.target : nullptr, rho, pm, (S*)pool));
    // ---- pass 1: C'_i from xcoms (array 0), Th'_l from theta (array 1)
    int n1 = m + s.ky;
    void* s1;
    RC(scratch(c, "rlc.s1", N * n1 * Z::COM1, &s1));
    {
      SidePlan sp;
      sp.tm = c->endo ? 4 : 1;  // endo = 0: one plain double-and-add lane per term ("k_var.plain"), as everywhere else
      ComOutputs{sp}.add(n1, 0, 0,
                         [&](int q, int b, ComOutputs& o) { rho_comb(o, pm, b, q < m ? 0 : 1, q < m ? q : q - m); });
      const ArrTab arrs = arr_tab({{0, v.xcoms, (uint32_t)(m * Z::COM1)}, {1, v.theta, (uint32_t)(s.ky * Z::COM1)}});
      const OutTab outs = out_tab(s1, (uint32_t)(n1 * Z::COM1));
      RC((run_side<C, F1>(c, ".r1", N, sp, arrs, (const S*)pool, pm.total, (const A1*)c->tabs->tab16_g1.p, outs)));
    }
    // ---- pass 2: elements 0..n-1 = P'_j, then [PB'] , U'_k (kx), [W1'] (MSMEG2).  Arrays: 0 = S1, 1 = A, 2 = target
    int iPB = n, iU = n + (s.yg ? 0 : 1), iW = iU + s.kx, n2 = iW + (ty == GS_MSMEG2 ? 1 : 0);
    void* s2;
    RC(scratch(c, "rlc.s2", N * n2 * Z::COM1, &s2));
    {
      SidePlan sp;
      sp.tm = c->endo ? 8 : 1;
      ComOutputs{sp}.add(n2, 0, 0, [&](int q, int b, ComOutputs& o) {
        if (q < n) {
          std::vector<VarTask> terms;
          head_terms(o, terms, pm, s, q, b, 1);
          com_terms(terms, pm.GC + q, n, m, 0, b);  // Gamma_ij C'_ib
          o.terms(terms);
        } else if (!s.yg && q == iPB) {
          emit_PB(o, pm, s, b, 0, 2);
        } else if (q < iW) {
          emit_U(o, pm, q - iU, b);
        } else {  // (MSMEG2)
          emit_W1(o, pm, b);
        }
      });
      const ArrTab arrs = arr_tab({{0, s1, (uint32_t)(n1 * Z::COM1)},
                                   {1, v.A, (uint32_t)(n * Z::G1), s.xg},
                                   {2, v.target, (uint32_t)Z::G1, ty == GS_MSMEG1}});
      const OutTab outs = out_tab(s2, (uint32_t)(n2 * Z::COM1));
      RC((run_side<C, F1>(c, ".r2", N, sp, arrs, (const S*)pool, pm.total, (const A1*)c->tabs->tab16_g1.p, outs)));
    }
    // ---- Miller: every G2 argument once.  P arrays: 0 = S2, 1 = S1.  Q arrays: q_arrays
    std::vector<PairRef> pr;
    for (int b = 0; b < 2; b++)
      add_pairs(pr,
                {{{0, 0}, {0, 0}, n, 0},                                    // (P'_j, d_j)
                 {{1, 0}, {1, 0, false}, s.yg ? m : 0, 0},                  // (C'_i, B_i)
                 {{0, iPB}, {2, 2}, s.yg ? 0 : 1, 0},                       // (PB', W2)
                 {{0, iU}, {3, 0}, s.kx, 1},                                // (-U'_k, pi_k)
                 {{1, m}, {2, 0}, s.ky, 1},                                 // (-Th'_l, v_l)
                 {{0, iW}, {4, 0, false}, ty == GS_MSMEG2 ? 1 : 0, 1}},     // (-W1', t)
                b, b);
    const ArrTab parr = arr_tab({{0, s2, (uint32_t)(n2 * Z::COM1)}, {1, s1, (uint32_t)(n1 * Z::COM1)}});
    const std::vector<MillerTask> mt = plan_miller_single(c, N, pr);
    *ntask_out = (int)mt.size();
    return miller_single(c, "rlc", N, mt, parr, q_arrays(c, v, false), mpart);
  }
  // acc[1] of a batched check: the product `t` of the targets' powers (PPE) or, with t null, the identity (built in `one`)
  static int put_acc1(gs_ctx* c, const GT* t, GT* one, void* acc) {
    if (!t) RC(launch(c, "k_gt_set_one", k_gt_set_one<C>, 1, 64, one));
    return launch(c, "k_gt_export", k_gt_export<C>, 1, 64, (size_t)1, t ? t : (const GT*)one, (uint8_t*)acc + Z::GT);
  }
  static int verify_rlc(gs_ctx* c, const VerifyIn& v, const uint64_t* rho, void* acc) {
    const size_t N = v.N;
    void *mpart, *pt, *tmp;
    int ntask;
    RC(rlc_front(c, v, rho, &mpart, &ntask));
    RC(scratch(c, "rlc.t", (N + 1) * sizeof(GT), &pt));
    RC(scratch(c, "rlc.tmp", (N * ntask / 4 + 8) * sizeof(GT), &tmp));
    RC(gt_product(c, N * ntask, (GT*)mpart, (GT*)tmp, (uint8_t*)acc));
    if (v.sh.ty != GS_PPE) return put_acc1(c, nullptr, (GT*)pt, acc);
    RC(launch(c, "k_rlc_tpow", k_rlc_tpow<C>, N, 64, N, (const uint8_t*)v.target, rho, (GT*)pt));
    return gt_product(c, N, (GT*)pt, (GT*)tmp, (uint8_t*)acc + Z::GT);
  }

  // Sum, across the `rows` rows of a device array, of the first `count` Com-shaped elements of every row (group F):
  // K-ary levels of k_batch_sum (K = 8) down to one row of Jacobian partials, then k_red: `count` normalised elements
  // at `out`, one shared inversion per lane.
  template <class F>
  static int batch_sum(gs_ctx* c, const std::string& tag, size_t rows, int count, const void* in, uint32_t row_bytes,
                       void* out) {
    const int K = 8, cols = 2 * count;
    const size_t com = 2 * AFFB(C, F);
    void *b0, *b1;
    const size_t r1 = (rows + K - 1) / K;
    RC(scratch(c, (tag + ".l0").c_str(), r1 * cols * sizeof(Jac<F>), &b0));
    RC(scratch(c, (tag + ".l1").c_str(), ((r1 + K - 1) / K) * cols * sizeof(Jac<F>), &b1));
    const std::string kn = "k_batch_sum" + tag;
    const Jac<F>* cur = nullptr;
    Jac<F>*dst = (Jac<F>*)b0, *other = (Jac<F>*)b1;
    for (size_t len = rows;;) {  // (a single row still goes through level 0: affine in, Jacobian out)
      const size_t lo = (len + K - 1) / K, total = lo * cols;
      c->work_hint = len * (uint64_t)cols;  // points summed
      RC((launch_seg<k_batch_sum<C, F>>(c, kn.c_str(), total, 64, total, len, cols, cur ? nullptr : (const uint8_t*)in,
                                        row_bytes, cur, dst, K)));
      cur = dst;
      std::swap(dst, other);
      len = lo;
      if (len == 1) break;
    }
    RedLaunch r;
    r.name = "k_red" + tag;
    r.tag = tag;
    for (int q = 0; q < count; q++) r.hred.push_back(mkred(2 * q, 2 * q + 1, 2 * q + 1, 2 * q + 2, 0, q));
    r.part = cur;
    r.nred = r.hred.size();
    r.nslots = cols;
    r.outs = out_tab(out, (uint32_t)(count * com));
    return run_red<C, F>(c, 1, r);
  }

  // N proofs of ONE equation: the constants A, B, Gamma, target exist once, so the random linear
  // combination is taken ACROSS the proofs before pairing wherever the other argument of a pair is a constant or a CRS
  // element.  In the notation of rlc_front (C'_e,ib, Th'_e,lb per proof e; r_ab = sum_e rho_e,ab):
  //   per proof   e(P'_e,jb, d_e,j.b),  P'_e,jb = rho_e,1b A_j + sum_i Gamma_ij C'_e,ib       2n pairs
  //               [eq_pi = 0: e(-U'_e,kb, pi_e,k.b), U'_e,kb = rho_e,0b u_k.0 + rho_e,1b u_k.1   2kx pairs]
  //   per batch   e(sum_e C'_e,i1, B_i)  |  e(PB_b, W2.b),  PB_b = sum_i b_i sum_e C'_e,ib [- r_1b t] [- sum_a r_ab t W1.a]
  //               [eq_pi = 1: e(-u_k.a, sum_e sum_b rho_e,ab pi_e,k.b)]
  //               e(-sum_e Th'_e,lb, v_l.b)      [MSMEG2: e(-(r_01 W1.0 + r_11 W1.1), t)]      target: t^(r_11)
  // Scalars: a pool per proof (rho, a_j rho) and ONE shared pool (Gamma, b, r, -t r), which the per-proof pass over
  // Gamma reads with a pool stride of 0.  So that this pass needs shared scalars only, rho_e,1b A_j (a_j rho_e,ab W1.a)
  // is an output of pass 1 and enters P' as the affine addend of a fixed-base lane without fixed-base terms.
  static int verify_eq_rlc(gs_ctx* c, const VerifyIn& v, const uint64_t* rho, void* acc) {
    const Shape& s = v.sh;
    const int ty = s.ty, m = s.m, n = s.n, kx = s.kx, ky = s.ky;
    const bool xg = s.xg, yg = s.yg;
    const size_t N = v.N;
    // planned: pi per proof, as measured at 2^14 for PPE and QuadEqu; folded in G2 where a proof has two pi elements and
    // the batch has 2^16 proofs or more (the fold is ahead there for PPE; profiles/eq_rlc/rate.json)
    const bool fold_pi = c->eq_pi >= 0 ? c->eq_pi == 1 : (kx == 2 && N >= ((size_t)1 << 16));
    RangeGuard rg_all("gs.verify_eq_rlc");
    // per proof, shared
    const PoolMap pp = pool_layout({{&PoolMap::RH, 4}, {&PoolMap::AR, xg ? 0 : 4 * n}});
    const PoolMap ps = pool_layout({{&PoolMap::GC, m * n}, {&PoolMap::BC, m}, {&PoolMap::RH, 4}, {&PoolMap::NR, 4}});
    void *pool, *spool, *sums;
    RC(scratch(c, "eqrlc.pool", N * pp.total * sizeof(S), &pool));
    RC(scratch(c, "eqrlc.spool", ps.total * sizeof(S), &spool));
    RC(scratch(c, "eqrlc.sums", 8 * sizeof(unsigned long long), &sums));
    HIPCHK(c, hipMemsetAsync(sums, 0, 8 * sizeof(unsigned long long), c->cur ? c->cur : c->stream));
    RC(launch(c, "k_prep_verify_eq_rlc", k_prep_verify_eq_rlc<C>, (N + 63) / 64 * 64, 64, N, n,
              xg ? nullptr : (const S*)v.A, rho, pp, (S*)pool, (unsigned long long*)sums));
    {
      const size_t lanes = std::max((size_t)m * n, (size_t)1);
      RC(launch(c, "k_prep_verify_eq_rlc.shared", k_prep_verify_eq_rlc_shared<C>, lanes, 64, m, n, (const S*)v.G,
                yg ? nullptr : (const S*)v.B, ty == GS_QUAD ? (const S*)v.target : nullptr,
                (const unsigned long long*)sums, ps, (S*)spool));
    }
    // terms per Straus lane: "var_tm" forces it; endo = 0: one plain double-and-add lane per term, as everywhere else
    auto TM = [&](int planned) { return !c->endo ? 1 : c->var_tm > 0 ? c->var_tm : planned; };
    // ---- pass 1 (per proof): C'_i (m), Th'_l (ky), RA_j = rho_1b A_j | sum_a a_j rho_ab W1.a (n), [U'_k (kx)]
    const int iTh = m, iRA = m + ky, iU = iRA + n, n1 = iU + (fold_pi ? 0 : kx);
    void* s1;
    RC(scratch(c, "eqrlc.s1", N * n1 * Z::COM1, &s1));
    {
      SidePlan sp;
      sp.tm = TM(4);
      ComOutputs{sp}.add(n1, 0, 0, [&](int q, int b, ComOutputs& o) {
        if (q < iRA) {
          rho_comb(o, pp, b, q < m ? 0 : 1, q < m ? q : q - m);
        } else if (q < iU) {
          std::vector<VarTask> terms;
          head_terms(o, terms, pp, s, q - iRA, b, 2);
          o.terms(terms);
        } else {
          emit_U(o, pp, q - iU, b);
        }
      });
      const ArrTab arrs =
          arr_tab({{0, v.xcoms, (uint32_t)(m * Z::COM1)}, {1, v.theta, (uint32_t)(ky * Z::COM1)}, {2, v.A, 0, xg}});
      const OutTab outs = out_tab(s1, (uint32_t)(n1 * Z::COM1));
      RC((run_side<C, F1>(c, ".q1", N, sp, arrs, (const S*)pool, pp.total, (const A1*)c->tabs->tab16_g1.p, outs)));
    }
    // ---- pass 2 (per proof, shared scalars): P'_j = RA_j + sum_i Gamma_ij C'_i
    void* s2;
    RC(scratch(c, "eqrlc.s2", N * n * Z::COM1, &s2));
    {
      SidePlan sp;
      sp.tm = TM(8);
      ComOutputs{sp}.add(n, 0, 0, [&](int j, int b, ComOutputs& o) {
        std::vector<VarTask> terms;
        com_terms(terms, ps.GC + j, n, m, 0, b);
        o.fix(0, 0xFF, 0, 0xFF, 0, 2 * (iRA + j) + b);
        o.terms(terms);
      });
      const ArrTab arrs = arr_tab({{0, s1, (uint32_t)(n1 * Z::COM1)}});
      const OutTab outs = out_tab(s2, (uint32_t)(n * Z::COM1));
      RC((run_side<C, F1>(c, ".q2", N, sp, arrs, (const S*)spool, 0, (const A1*)c->tabs->tab16_g1.p, outs)));
    }
    // ---- across the batch: sum_e C'_e,i and sum_e Th'_e,l (the first m + ky elements of every row of s1)
    void* ssum;
    RC(scratch(c, "eqrlc.ssum", (m + ky) * Z::COM1, &ssum));
    RC(batch_sum<F1>(c, ".eqs1", N, m + ky, s1, (uint32_t)(n1 * Z::COM1), ssum));
    // ---- folded pi: Pi_e,k.a = sum_b rho_e,ab pi_e,k.b per proof (short terms), then their sum in G2
    void* pisum = nullptr;
    if (fold_pi) {
      void* s3;
      RC(scratch(c, "eqrlc.s3", N * kx * Z::COM2, &s3));
      SidePlan sp;
      sp.tm = TM(8);
      ComOutputs{sp}.add(kx, 0, 0, [&](int k, int a, ComOutputs& o) {
        o.terms({mkvar(pp.RH + 2 * a, 0, 2 * k, 0), mkvar(pp.RH + 2 * a + 1, 0, 2 * k + 1, 0)});
      });
      const ArrTab arrs = arr_tab({{0, v.pi, (uint32_t)(kx * Z::COM2)}});
      const OutTab outs = out_tab(s3, (uint32_t)(kx * Z::COM2));
      RC((run_side<C, F2>(c, ".q3", N, sp, arrs, (const S*)pool, pp.total, (const A2*)c->tabs->tab16_g2.p, outs)));
      RC(scratch(c, "eqrlc.pisum", kx * Z::COM2, &pisum));
      RC(batch_sum<F2>(c, ".eqs2", N, kx, s3, (uint32_t)(kx * Z::COM2), pisum));
    }
    // ---- batch-level G1 outputs (one "equation", shared pool): [PB] (scalar b), [W1'] (MSMEG2)
    const int iPB = 0, iW = yg ? 0 : 1, nb = iW + (ty == GS_MSMEG2 ? 1 : 0);
    void* sb = nullptr;
    if (nb) {
      RC(scratch(c, "eqrlc.sb", nb * Z::COM1, &sb));
      SidePlan sp;
      sp.tm = yg ? 1 : TM(8);  // (MSMEG2's only output has no variable-base term)
      ComOutputs{sp}.add(nb, 0, 0, [&](int q, int b, ComOutputs& o) {
        if (!yg && q == iPB)
          emit_PB(o, ps, s, b, 0, 1);  // over sum_e C'_e,i, with r_ab for rho_ab
        else
          emit_W1(o, ps, b);
      });
      const ArrTab arrs = arr_tab({{0, ssum, 0}, {1, v.target, 0, ty == GS_MSMEG1}});
      const OutTab outs = out_tab(sb, (uint32_t)(nb * Z::COM1));
      RC((run_side<C, F1>(c, ".q4", 1, sp, arrs, (const S*)spool, 0, (const A1*)c->tabs->tab16_g1.p, outs)));
    }
    // ---- Miller.  Per proof: P arrays 0 = s2, 1 = s1; Q arrays 0 ycoms, 3 pi
    // per batch: P arrays 0 = sb, 1 = ssum, 2 = crs G1 (u, W1); Q arrays 1 B, 2 crs G2 (v, W2), 3 = pisum, 4 target
    std::vector<PairRef> pr, prb;
    for (int b = 0; b < 2; b++)
      add_pairs(pr,
                {{{0, 0}, {0, 0}, n, 0},                           // (P'_e,j, d_e,j)
                 {{1, iU}, {3, 0}, fold_pi ? 0 : kx, 1}},          // (-U'_e,k, pi_e,k)
                b, b);
    for (int b = 0; b < 2; b++)
      add_pairs(prb,
                {{{1, 0}, {1, 0, false}, yg ? m : 0, 0},                    // (sum_e C'_e,i, B_i)
                 {{0, iPB}, {2, 2}, yg ? 0 : 1, 0},                         // (PB, W2)
                 {{1, iTh}, {2, 0}, ky, 1},                                 // (-sum_e Th'_e,l, v_l)
                 {{2, 0}, {3, 0}, fold_pi ? kx : 0, 1},                     // (-u_k.a, Pi_k.a), a = b here
                 {{0, iW}, {4, 0, false}, ty == GS_MSMEG2 ? 1 : 0, 1}},     // (-W1', t)
                b, b);
    const std::vector<MillerTask> mt = plan_miller_single(c, N, pr), mtb = plan_miller_single(c, 1, prb);
    const int ntask = (int)mt.size(), ntb = (int)mtb.size();
    const size_t nparts = N * ntask + ntb;
    void *mpart, *tmp, *pt;
    RC(scratch(c, "eqrlc.mpart", nparts * sizeof(GT), &mpart));
    RC(scratch(c, "eqrlc.tmp", (nparts / 4 + 8) * sizeof(GT), &tmp));
    RC(scratch(c, "eqrlc.t", sizeof(GT), &pt));
    {
      const MillerTask *dmt, *dmtb;
      RC(upload(c, "eqrlc.mt", mt, &dmt));
      RC(upload(c, "eqrlc.mtb", mtb, &dmtb));
      const ArrTab parr = arr_tab({{0, s2, (uint32_t)(n * Z::COM1)}, {1, s1, (uint32_t)(n1 * Z::COM1)}});
      const ArrTab qarr = arr_tab({{0, v.ycoms, (uint32_t)(n * Z::COM2)}, {3, v.pi, (uint32_t)(kx * Z::COM2)}});
      // the batch-level pairs are one wave: they ride along as a second segment of the per-proof launch (a launch of
      // their own would add a serial Miller lane to every call: k_miller.eqrlc.batch in profiles/eq_rlc/rate.json)
      miller_work_hint(c, N, mt, false);
      const LaunchRec per = seg_rec<k_miller<C, false>>(c, "k_miller.eqrlc", N * ntask, 64, N * ntask, ntask, dmt, parr,
                                                        qarr, (GT*)mpart, 1, lines(c));
      const ArrTab parb = arr_tab({{0, sb, 0, nb > 0}, {1, ssum, 0}, {2, c->tabs->crs_g1.p, 0}});
      const ArrTab qarb =
          arr_tab({{1, v.B, 0, yg}, {2, c->tabs->crs_g2.p, 0}, {3, pisum, 0, fold_pi}, {4, v.target, 0, ty == GS_MSMEG2}});
      miller_work_hint(c, 1, mtb, false);
      const LaunchRec bat = seg_rec<k_miller<C, false>>(c, "k_miller.eqrlc.batch", (size_t)ntb, 64, (size_t)ntb, ntb, dmtb,
                                                        parb, qarb, (GT*)mpart + N * ntask, 1, lines(c));
      RC(seg_pair(c, bat, per));  // (the single wave in the first block of the grid)
    }
    RC(gt_product(c, nparts, (GT*)mpart, (GT*)tmp, (uint8_t*)acc));
    if (ty == GS_PPE)
      RC(launch(c, "k_eq_rlc_tpow", k_eq_rlc_tpow<C>, 1, 64, (const uint8_t*)v.target, (const S*)spool + ps.RH + 3,
                (GT*)pt));
    return put_acc1(c, ty == GS_PPE ? (const GT*)pt : nullptr, (GT*)pt, acc);
  }

  // The batched verifier with fault localisation.  Same front; the products are a K-ary tree whose
  // levels are KEPT: level 0 = the N leaves (f_e, t_e), level l = products of runs of K of level l - 1, one node at the
  // top.  The descent then runs from the root down, one launch per level, each sized for the whole level: the frontier
  // (failing nodes of the level above, and how many) is device memory, so nothing here waits for the device.
  //   rlc.lvl.f / rlc.lvl.t   the levels, one after the other (t only for PPE: it is one everywhere else)
  //   rlc.frontier            u32: counts[0 .. L + 1] (failing nodes per level; [L + 1] = 1, the root's virtual parent),
  //                           then the lists of levels 1 .. L and the virtual parent's list {0}
  static int verify_rlc_locate(gs_ctx* c, const VerifyIn& v, const uint64_t* rho, void* acc, uint8_t* ok, uint32_t* info) {
    const size_t N = v.N;
    void* mpart;
    int ntask;
    RC(rlc_front(c, v, rho, &mpart, &ntask));
    const int K = c->locate_k ? c->locate_k : 8;  // planned: the arity of gt_product
    const bool ppe = v.sh.ty == GS_PPE;
    std::vector<size_t> cnt{N}, off{0};
    while (cnt.back() > 1) {
      off.push_back(off.back() + cnt.back());
      cnt.push_back((cnt.back() + K - 1) / K);
    }
    const int L = (int)cnt.size() - 1;
    const size_t nodes = off[L] + 1;
    void *lf, *lt = nullptr, *fr;
    RC(scratch(c, "rlc.lvl.f", nodes * sizeof(GT), &lf));
    if (ppe) RC(scratch(c, "rlc.lvl.t", nodes * sizeof(GT), &lt));
    const size_t hdr = (size_t)L + 2, fr_words = hdr + (nodes - N) + 1;
    RC(scratch(c, "rlc.frontier", fr_words * sizeof(uint32_t), &fr));
    GT *F = (GT*)lf, *T = (GT*)lt;
    uint32_t* count = (uint32_t*)fr;
    auto list = [&](int l) { return count + hdr + (l > L ? nodes - N : off[l] - N); };  // l = 1 .. L + 1
    hipStream_t st = c->cur ? c->cur : c->stream;
    HIPCHK(c, hipMemsetAsync(fr, 0, fr_words * sizeof(uint32_t), st));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)(count + L + 1), 1, 1, st));
    HIPCHK(c, hipMemsetAsync(ok, 1, N, st));
    HIPCHK(c, hipMemsetAsync(info, 0, 2 * sizeof(uint32_t), st));
    // ---- the levels
    RC(launch(c, "k_rlc_leaf", k_rlc_leaf<C>, N, 64, N, ntask, (const GT*)mpart, F));
    if (ppe) RC(launch(c, "k_rlc_tpow", k_rlc_tpow<C>, N, 64, N, (const uint8_t*)v.target, rho, T));
    for (int l = 1; l <= L; l++) {
      const size_t half = (cnt[l] + 63) / 64 * 64;
      RC(launch(c, "k_rlc_tree", k_rlc_tree<C>, ppe ? half + cnt[l] : cnt[l], 64, cnt[l - 1], (const GT*)(F + off[l - 1]),
                (const GT*)(ppe ? T + off[l - 1] : nullptr), cnt[l], F + off[l], ppe ? T + off[l] : nullptr, K));
    }
    RC(launch(c, "k_gt_export", k_gt_export<C>, 1, 64, (size_t)1, (const GT*)(F + off[L]), (uint8_t*)acc));
    void* one = nullptr;
    if (!ppe) RC(scratch(c, "rlc.one", sizeof(GT), &one));
    RC(put_acc1(c, ppe ? T + off[L] : nullptr, (GT*)one, acc));
    // ---- the descent: level L is the root under its virtual parent, level 0 the leaves
    for (int l = L; l >= 0; l--) {
      LocateLevel lv;
      lv.fr_in = list(l + 1);
      lv.cnt_in = count + l + 1;
      lv.fr_out = l ? list(l) : nullptr;
      lv.cnt_out = l ? count + l : nullptr;
      lv.n_child = (uint32_t)cnt[l];
      lv.fan = l == L ? 1 : K;
      lv.ok = l ? nullptr : ok;
      lv.info = info;
      const size_t items = l == L ? 1 : cnt[l + 1] * (size_t)K;
      const GT *Fl = F + off[l], *Tl = ppe ? T + off[l] : nullptr;
      if (coop_lanes(c, items))  // (the level's own launch: not fillN)
        RC(launch(c, "k_rlc_locate.coop", k_rlc_locate_coop<C>, (items + 20) / 21 * 63, 63, lv, Fl, Tl));
      else
        RC(launch(c, "k_rlc_locate", k_rlc_locate<C>, items, 64, lv, Fl, Tl));
    }
    return GS_OK;
  }

  // Statement-batched verifier: S statements of E equations each over ONE set of commitments per statement.  The
  // random linear combination is taken ACROSS the equations of a statement before anything is paired (Blazy et al.,
  // ACNS 2010), so a statement costs 2n + 2m + 2kx + 2ky Miller pairs whatever E is:
  //   G1 pass (Com1-shaped outputs, component b):
  //     P_j.b   = sum_e rho_e,1b A_ej + sum_i,a g_ab,ij c_i.a          (sum_a (sum_e rho_e,ab a_ej) W1.a for scalar A)
  //     PB.b    = sum_i,a (sum_e rho_e,ab b_ei) c_i.a [- sum_e rho_e,1b t_e] [- sum_a (sum_e rho_e,ab t_e) W1.a]
  //     Th_l.b  = sum_e,a rho_e,ab theta_el.a
  //   G2 pass (Com2-shaped outputs, component a):
  //     Q_i.a   = sum_e rho_e,a1 B_ei,   Pi_k.a = sum_e,b rho_e,ab pi_ek.b,   T.a = sum_e rho_e,a1 t_e  (MSMEG2)
  //   pairs: e(P_j.b, d_j.b)  e(c_i.a, Q_i.a) | e(PB.b, W2.b)  e(-u_k.a, Pi_k.a)  e(-Th_l.b, v_l.b)  [e(-W1.a, T.a)]
  // The engine's unit is the statement (N := S): array strides are per statement, p_idx runs over (e, j).  Short
  // (64-bit) and full-size terms go to separate Straus lanes, so the short ones skip their leading windows; outputs
  // over the same bases (the two components of every output above) share a table build (share_tables).
  // v.N: the statements
  static int verify_stmt_rlc(gs_ctx* c, const VerifyIn& v, size_t E_, const uint64_t* rho, void* acc, uint8_t* ok) {
    const Shape& s = v.sh;
    const int ty = s.ty, m = s.m, n = s.n, kx = s.kx, ky = s.ky, E = (int)E_;
    const bool xg = s.xg, yg = s.yg;
    const size_t S = v.N;
    RangeGuard rg_all("gs.verify_stmt_rlc");
    const PoolMap pm = pool_layout({{&PoolMap::RH, 4 * E}, {&PoolMap::GC, 4 * m * n}, {&PoolMap::AR, xg ? 0 : 4 * n},
                                    {&PoolMap::BC, yg ? 0 : 4 * m}, {&PoolMap::NR, ty == GS_QUAD ? 4 : 0}});
    const int nout = pm.total;
    void* pool;
    RC(scratch(c, "srlc.pool", S * pm.total * sizeof(Fr<C>), &pool));
    {
      // one lane per statement while a statement is small; one lane per output scalar (E products each) otherwise
      // (4 x 4, S E = 2^14, profiles/stmt_rlc/rate_2p14.json: lanes of E products take 0.07 ms at E = 16 and 0.15 ms at
      // E = 64; one lane per statement walking the 1664 products of an E = 16 statement was an order of magnitude slower)
      const bool narrow = !wide_prep(m, n) && (size_t)E * (size_t)(4 * m * n + 4 * (m + n) + 8) <= 128;
      const int per = narrow ? 1 : nout;
      c->work_hint = S * (uint64_t)E * (uint64_t)(nout - 4 * E + 4);
      RC(launch(c, "k_prep_verify_stmt_rlc", k_prep_verify_stmt_rlc<C>, S * (size_t)per, 64, S, E, m, n, nout, per,
                (const Fr<C>*)v.G, xg ? nullptr : (const Fr<C>*)v.A, yg ? nullptr : (const Fr<C>*)v.B,
                ty == GS_QUAD ? (const Fr<C>*)v.target : nullptr, rho, pm, (Fr<C>*)pool));
    }
    auto RH = [&](int e, int a, int b) { return pm.RH + 4 * e + 2 * a + b; };
    const int tm = c->endo ? 8 : 1;  // endo = 0: one plain double-and-add lane per term, as everywhere else
    // ---- G1 pass: elements 0..n-1 = P_j, then [PB], Th_l (ky).  Arrays: 0 xcoms, 1 A, 2 target (MSMEG1), 3 theta
    const int iPB = n, iTh = n + (yg ? 0 : 1), n1 = iTh + ky;
    void* s1;
    RC(scratch(c, "srlc.s1", S * n1 * Z::COM1, &s1));
    {
      SidePlan sp;
      sp.tm = tm;
      ComOutputs{sp}.add(n1, 0, 0, [&](int q, int b, ComOutputs& o) {
        std::vector<VarTask> shortt, full;
        if (q < n) {
          const int j = q;
          if (xg)
            for (int e = 0; e < E; e++) shortt.push_back(mkvar(RH(e, 1, b), 1, e * n + j, 0));
          else
            rho_fix(o, pm.AR + j * 4, b, tb_w(0), tb_w(1));
          for (int i = 0; i < m; i++)
            for (int a = 0; a < 2; a++) full.push_back(mkvar(pm.GC + ((2 * a + b) * m + i) * n + j, 0, 2 * i + a, 0));
        } else if (!yg && q == iPB) {
          for (int i = 0; i < m; i++)
            for (int a = 0; a < 2; a++) full.push_back(mkvar(pm.BC + i * 4 + 2 * a + b, 0, 2 * i + a, 0));
          if (ty == GS_MSMEG1)
            for (int e = 0; e < E; e++) {
              VarTask v = mkvar(RH(e, 1, b), 2, e, 0);
              v.neg = 1;
              shortt.push_back(v);
            }
          if (ty == GS_QUAD) rho_fix(o, pm.NR, b, tb_w(0), tb_w(1));
        } else {
          const int l = q - iTh;
          for (int e = 0; e < E; e++)
            for (int a = 0; a < 2; a++) shortt.push_back(mkvar(RH(e, a, b), 3, 2 * (e * ky + l) + a, 0));
        }
        o.terms(shortt);
        o.terms(full);
      });
      const ArrTab arrs = arr_tab({{0, v.xcoms, (uint32_t)(m * Z::COM1)},
                                   {1, v.A, (uint32_t)((size_t)E * n * Z::G1), xg},
                                   {2, v.target, (uint32_t)((size_t)E * Z::G1), ty == GS_MSMEG1},
                                   {3, v.theta, (uint32_t)((size_t)E * ky * Z::COM1)}});
      const OutTab outs = out_tab(s1, (uint32_t)(n1 * Z::COM1));
      RC((run_side<C, F1>(c, ".s1", S, sp, arrs, (const Fr<C>*)pool, pm.total, (const A1*)c->tabs->tab16_g1.p, outs)));
    }
    // ---- G2 pass: elements [Q_i (m)], Pi_k (kx), [T] (MSMEG2).  Arrays: 0 B, 1 pi, 2 target (MSMEG2)
    const int iPi = yg ? m : 0, iT = iPi + kx, n2 = iT + (ty == GS_MSMEG2 ? 1 : 0);
    void* s2;
    RC(scratch(c, "srlc.s2", S * n2 * Z::COM2, &s2));
    {
      SidePlan sp;
      sp.tm = tm;
      ComOutputs{sp}.add(n2, 0, 0, [&](int q, int a, ComOutputs& o) {
        std::vector<VarTask> terms;
        if (q < iPi) {
          for (int e = 0; e < E; e++) terms.push_back(mkvar(RH(e, a, 1), 0, e * m + q, 0));
        } else if (q < iT) {
          const int k = q - iPi;
          for (int e = 0; e < E; e++)
            for (int b = 0; b < 2; b++) terms.push_back(mkvar(RH(e, a, b), 1, 2 * (e * kx + k) + b, 0));
        } else {
          for (int e = 0; e < E; e++) terms.push_back(mkvar(RH(e, a, 1), 2, e, 0));
        }
        o.terms(terms);
      });
      const ArrTab arrs = arr_tab({{0, v.B, (uint32_t)((size_t)E * m * Z::G2), yg},
                                   {1, v.pi, (uint32_t)((size_t)E * kx * Z::COM2)},
                                   {2, v.target, (uint32_t)((size_t)E * Z::G2), ty == GS_MSMEG2}});
      const OutTab outs = out_tab(s2, (uint32_t)(n2 * Z::COM2));
      RC((run_side<C, F2>(c, ".s2", S, sp, arrs, (const Fr<C>*)pool, pm.total, (const A2*)c->tabs->tab16_g2.p, outs)));
    }
    // ---- Miller.  P arrays: 0 = S1, 1 = xcoms, 2 = crs G1 (u, W1).  Q arrays: 0 ycoms, 1 = S2, 2 = crs G2 (v, W2)
    std::vector<PairRef> pr;
    for (int b = 0; b < 2; b++)
      add_pairs(pr,
                {{{0, 0}, {0, 0}, n, 0},                   // (P_j.b, d_j.b)
                 {{0, iPB}, {2, 2}, yg ? 0 : 1, 0},        // (PB.b, W2.b)
                 {{0, iTh}, {2, 0}, ky, 1}},               // (-Th_l.b, v_l.b)
                b, b);
    for (int a = 0; a < 2; a++)
      add_pairs(pr,
                {{{1, 0}, {1, 0}, yg ? m : 0, 0},                      // (c_i.a, Q_i.a)
                 {{2, 0}, {1, iPi}, kx, 1},                            // (-u_k.a, Pi_k.a)
                 {{2, 2}, {1, iT}, ty == GS_MSMEG2 ? 1 : 0, 1}},       // (-W1.a, T.a)
                a, a);
    const std::vector<MillerTask> mt = plan_miller_single(c, S, pr);
    const int ntask = (int)mt.size();
    const ArrTab parr =
        arr_tab({{0, s1, (uint32_t)(n1 * Z::COM1)}, {1, v.xcoms, (uint32_t)(m * Z::COM1)}, {2, c->tabs->crs_g1.p, 0}});
    const ArrTab qarr =
        arr_tab({{0, v.ycoms, (uint32_t)(n * Z::COM2)}, {1, s2, (uint32_t)(n2 * Z::COM2)}, {2, c->tabs->crs_g2.p, 0}});
    void* mpart;
    RC(miller_single(c, "srlc", S, mt, parr, qarr, &mpart));
    // ---- PPE: T_s = prod_e t_e^rho_e,11 (segmented K-ary product of k_rlc_tpow's S E powers)
    const GT* tprod = nullptr;
    if (ty == GS_PPE) {
      const int K = 8;
      void *t0, *t1;
      RC(scratch(c, "srlc.t0", S * (size_t)E * sizeof(GT), &t0));
      RC(scratch(c, "srlc.t1", S * (((size_t)E + K - 1) / K) * sizeof(GT), &t1));
      RC(launch(c, "k_rlc_tpow", k_rlc_tpow<C>, S * (size_t)E, 64, S * (size_t)E, (const uint8_t*)v.target, rho, (GT*)t0));
      GT *in = (GT*)t0, *out = (GT*)t1;
      for (size_t len = (size_t)E; len > 1;) {
        size_t lo = (len + K - 1) / K;
        RC(launch(c, "k_gt_prod_seg", k_gt_prod_seg<C>, S * lo, 64, S, len, (const GT*)in, lo, out, K));
        std::swap(in, out);
        len = lo;
      }
      tprod = in;
    }
    // ---- one final exponentiation per statement
    if (coop_lanes(c, fillN(c, S)))
      RC(launch_seg<k_stmt_final_coop<C>>(c, "k_stmt_final.coop", (S + 20) / 21 * 63, 63, S, ntask, (const GT*)mpart, tprod,
                (uint8_t*)acc, ok));
    else
      RC(launch_seg<k_stmt_final<C>>(c, "k_stmt_final", S, 64, S, ntask, (const GT*)mpart, tprod, (uint8_t*)acc, ok));
    return GS_OK;
  }

  // accs: count boundary-form pairs (host).  ok = FE(prod accs[i][0]) == prod accs[i][1]
  // accs: `count` interleaved pairs (f_i, t_i) in boundary form, on the host or (dev) on this context's device
  static int gt_finalize(gs_ctx* c, size_t count, const void* accs_host, uint8_t* ok_host, bool dev = false) {
    void *raw, *d, *t, *two, *dok, *twob;
    RC(scratch(c, "fin.raw", 2 * count * Z::GT, &raw));
    RC(scratch(c, "fin.in", 2 * count * sizeof(GT), &d));
    RC(scratch(c, "fin.tmp", (count + 8) * sizeof(GT), &t));
    RC(scratch(c, "fin.two", 2 * sizeof(GT), &two));
    RC(scratch(c, "fin.twob", 2 * Z::GT, &twob));
    RC(scratch(c, "fin.ok", 16, &dok));
    // de-interleave: [f0 f1 ...][t0 t1 ...]
    const uint8_t* src = (const uint8_t*)accs_host;
    if (dev) {  // two strided device-to-device copies on the context's stream
      HIPCHK(c, hipMemcpy2DAsync(raw, Z::GT, src, 2 * Z::GT, Z::GT, count, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpy2DAsync((uint8_t*)raw + count * Z::GT, Z::GT, src + Z::GT, 2 * Z::GT, Z::GT, count,
                                 hipMemcpyDeviceToDevice, c->stream));
    } else {
      std::vector<uint8_t> h(2 * count * Z::GT);
      for (size_t i = 0; i < count; i++) {
        memcpy(&h[i * Z::GT], src + (2 * i) * Z::GT, Z::GT);
        memcpy(&h[(count + i) * Z::GT], src + (2 * i + 1) * Z::GT, Z::GT);
      }
      HIPCHK(c, hipStreamSynchronize(c->stream));
      HIPCHK(c, hipMemcpy(raw, h.data(), h.size(), hipMemcpyHostToDevice));
    }
    RC(launch(c, "k_gt_import", k_gt_import<C>, 2 * count, 64, 2 * count, (const uint8_t*)raw, (GT*)d));
    RC(gt_product(c, count, (GT*)d, (GT*)t, (uint8_t*)twob));
    RC(gt_product(c, count, (GT*)d + count, (GT*)t, (uint8_t*)twob + Z::GT));
    RC(launch(c, "k_gt_import", k_gt_import<C>, 2, 64, (size_t)2, (const uint8_t*)twob, (GT*)two));
    RC(launch(c, "k_fe_eq", k_fe_eq<C>, 3, 3, (const GT*)two, (uint8_t*)dok));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(ok_host, dok, 1, hipMemcpyDeviceToHost));
    return GS_OK;
  }
};

// ---------------------------------------------------------------------------
// dispatch helpers
// ---------------------------------------------------------------------------
#if defined(GS_ONLY_BLS)
// experiment builds (tools/build_variant.sh NAME -DGS_ONLY_BLS): half the compile time, BN254 calls fail
#define DISPATCH(ctx, EXPR) \
  ((ctx)->curve == GS_CURVE_BLS12_381 ? Impl<Bls12_381>::EXPR : fail(ctx, GS_ERR_ARG, "built with GS_ONLY_BLS"))
#else
#define DISPATCH(ctx, EXPR)                                   \
  ((ctx)->curve == GS_CURVE_BLS12_381 ? Impl<Bls12_381>::EXPR : Impl<Bn254>::EXPR)
#endif

#if defined(GS_ONLY_BLS)
#define DISPATCH_FN(ctx, FN, ARGS) \
  ((ctx)->curve == GS_CURVE_BLS12_381 ? FN<Bls12_381> ARGS : fail(ctx, GS_ERR_ARG, "built with GS_ONLY_BLS"))
#else
#define DISPATCH_FN(ctx, FN, ARGS) ((ctx)->curve == GS_CURVE_BLS12_381 ? FN<Bls12_381> ARGS : FN<Bn254> ARGS)
#endif

#if defined(GS_ONLY_BLS)
#define WIRE_DISPATCH(expr_bls, expr_bn) (c->curve == 0 ? (expr_bls) : fail(c, GS_ERR_ARG, "built with GS_ONLY_BLS"))
#else
#define WIRE_DISPATCH(expr_bls, expr_bn) (c->curve == 0 ? (expr_bls) : (expr_bn))
#endif

static size_t sz_fq(int curve) { return curve == 0 ? 4 * Bls12_381::N : 4 * Bn254::N; }
static const size_t SZ_FR = 32;

struct HostStage {  // host<->device staging for the un-suffixed entry points
  // Buffers come from the context's grow-only scratch map ("stage.<k>"): no hipMalloc / hipFree in steady state
  // (hipFree synchronises the device; per-call allocation cost 10-20 % of a 2^12 batch).
  gs_ctx* c;
  int k = 0;
  explicit HostStage(gs_ctx* ctx) : c(ctx) {}
  int slot(size_t bytes, void** d) {
    char name[32];
    snprintf(name, sizeof name, "stage.%d", k++);
    return scratch(c, name, bytes, d);
  }
  int in(const void* h, size_t bytes, void** d) {
    *d = nullptr;
    if (!h || bytes == 0) return GS_OK;
    RC(slot(bytes, d));
    hipError_t e = hipMemcpyAsync(*d, h, bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return fail(c, GS_ERR_DEVICE, "hipMemcpy H2D", e);
    return GS_OK;
  }
  int out(void* h, size_t bytes, void** d) {
    *d = nullptr;
    if (!h || bytes == 0) return GS_OK;
    return slot(bytes, d);
  }
  int back(void* h, const void* d, size_t bytes) {
    if (!h || bytes == 0) return GS_OK;
    hipError_t e = hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return fail(c, GS_ERR_DEVICE, "hipMemcpy D2H", e);
    e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, GS_ERR_DEVICE, "sync", e);
    return GS_OK;
  }
};
// The plain host form of a checked call: stage the inputs in, give every output a slot, run(d) on the device pointers
// (d[] holds the inputs' first, then the outputs', in the order listed), copy the outputs back.
struct HostBuf {
  const void* h;
  size_t bytes;
};
template <class Run>
static int staged_call(gs_ctx* c, std::initializer_list<HostBuf> ins, std::initializer_list<HostBuf> outs, Run run) {
  HostStage st(c);
  void* d[8];
  int k = 0;
  for (const HostBuf& b : ins) RC(st.in(b.h, b.bytes, &d[k++]));
  for (const HostBuf& b : outs) RC(st.out(const_cast<void*>(b.h), b.bytes, &d[k++]));
  RC(run(d));
  k = (int)ins.size();
  for (const HostBuf& b : outs) RC(st.back(const_cast<void*>(b.h), d[k++], b.bytes));
  return GS_OK;
}

// Forget the binding key.  The digit streams on the device are the only copy the context keeps.
static void clear_extraction_key(gs_ctx* c) {
  c->have_xkey = false;
  if (!c->xkey.p) return;
  hipSetDevice(c->device);
  drain_ctx(c);  // extractions already enqueued still read the streams
  // on the context's stream, and finished before this returns: a null-stream memset is ordered against nothing on a
  // non-blocking caller stream, where the next key's k_extract_key would race it
  hipMemsetAsync(c->xkey.p, 0, c->xkey.cap, c->stream);
  hipStreamSynchronize(c->stream);
}

// Forget the simulation trapdoor: the context's copy is zeroed on the stream, behind the simulations already enqueued.
static void clear_simulation_key(gs_ctx* c) {
  c->have_skey = false;
  if (!c->skey.p) return;
  hipSetDevice(c->device);
  drain_ctx(c);
  hipMemsetAsync(c->skey.p, 0, c->skey.cap, c->stream);
  hipStreamSynchronize(c->stream);
}

// Forget the generator's key: the context's copy is zeroed on the stream, behind the draws already enqueued.
static void clear_rand_key(gs_ctx* c) {
  c->have_rkey = false;
  if (!c->rkey.p) return;
  hipSetDevice(c->device);
  drain_ctx(c);
  hipMemsetAsync(c->rkey.p, 0, c->rkey.cap, c->stream);
  hipStreamSynchronize(c->stream);
}

static int check_ctx(gs_ctx* c, bool need_crs) {
  if (!c) return GS_ERR_ARG;
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail(c, GS_ERR_DEVICE, "hipSetDevice", e);
  if (need_crs && !c->have_crs) return fail(c, GS_ERR_NOCRS, "gs_set_crs has not been called");
  return GS_OK;
}

// Matrix<Com>::left_mul for a (k x 1) column: out[i] = sum_j lhs[i][j] col[j].
// Expressed through the engine as `rows` proof-like elements with var tasks on both components.
template <class C, class F>
static int left_mul_impl(gs_ctx* c, int rows, int k, const void* lhs, const void* col, void* out) {
  typedef Fr<C> S;
  size_t com = 2 * (sizeof(Aff<F>) == sizeof(Aff<Fq<C>>) ? Sz<C>::G1 : Sz<C>::G2);
  HostStage st(c);
  void *dl, *dc, *dout;
  RC(st.in(lhs, (size_t)rows * k * sizeof(S), &dl));
  RC(st.in(col, (size_t)k * com, &dc));
  RC(st.out(out, (size_t)rows * com, &dout));
  // pool = canonical lhs via k_prep_verify (m*n scalars)
  const PoolMap pm = pool_layout({{&PoolMap::GC, rows * k}});
  void* pool;
  RC(scratch(c, "lm.pool", (size_t)pm.total * sizeof(S), &pool));
  RC(launch_seg<k_prep_verify<C>>(c, "k_prep_verify", 1, 64, (size_t)1, rows, k, (const S*)dl, (const S*)nullptr,
            (const S*)nullptr, (const S*)nullptr, pm, (S*)pool));
  // Planned: one term per lane (k_var).  The forced Straus shapes are honoured so that the lanes can be driven with
  // chosen bases and scalars: var_tm > 1 groups the k terms of a component (all rows run over the same 2 k bases, so
  // share_tables gives var_mo outputs per lane), var_tab = 1 (G1) puts them on shared window tables of the 2 k bases.
  // endo = 0 keeps the plain lanes.
  SidePlan sp;
  if (c->endo && c->var_tab == 1 && std::is_same<F, Fq<C>>::value) {
    sp.tm = 8;
    sp.tab_bases = 2 * k;
  } else if (c->endo && c->var_tm > 1) {
    sp.tm = c->var_tm;
  }
  ComOutputs outp{sp};
  outp.add(rows, 0, 0, [&](int i, int a, ComOutputs& o) {
    std::vector<VarTask> terms;
    for (int j = 0; j < k; j++) terms.push_back(mkvar(i * k + j, 0, 2 * j + a, 0));
    o.terms(terms);
  });
  RC((run_side<C, F>(c, ".lm", 1, sp, arr_tab({{0, dc, 0}}), (const S*)pool, pm.total, (const Aff<F>*)nullptr,
                     out_tab(dout, 0))));
  return st.back(out, dout, (size_t)rows * com);
}

// Matrix<Fr> product through the prover's own scalar-preparation kernel: with R = lhs^T (inner x rows) and
// Gamma = rhs (inner x cols), Psi = R^T Gamma is lhs * rhs (prove.rs:133; the reference's Mat::right_mul / left_mul on
// Matrix<Fr>, data_structures.rs:824-912).  Shapes with inner * cols >= 1024 take the one-lane-per-output kernel.
template <class C> static int fr_matmul_impl(gs_ctx* c, int rows, int inner, int cols, const void* lhs, const void* rhs, void* out) {
  typedef Fr<C> S;
  std::vector<uint8_t> rt((size_t)inner * rows * sizeof(S));
  const uint8_t* a = (const uint8_t*)lhs;
  for (int k = 0; k < rows; k++)
    for (int i = 0; i < inner; i++) memcpy(&rt[((size_t)i * rows + k) * sizeof(S)], a + ((size_t)k * inner + i) * sizeof(S), sizeof(S));
  HostStage st(c);
  void *dR, *dG, *dout;
  RC(st.in(rt.data(), rt.size(), &dR));
  RC(st.in(rhs, (size_t)inner * cols * sizeof(S), &dG));
  RC(st.out(out, (size_t)rows * cols * sizeof(S), &dout));
  const int m = inner, n = cols, kx = rows, ky = 0;
  PoolMap pm = Impl<C>::prove_pool(m, n, kx, ky);
  void* pool;
  RC(scratch(c, "frmm.pool", (size_t)pm.total * sizeof(S), &pool));
  if (wide_prep(m, n)) {
    int W = m * kx + n * ky + ky * kx + m + n + kx * n + ky * m;
    RC(launch_seg<k_prep_prove_wide_a<C>>(c, "k_prep_prove.a", (size_t)W, 64, (size_t)W, W, m, n, kx, ky, (const S*)dG,
              (const S*)dR, (const S*)dR, (const S*)dR, (const S*)nullptr, (const S*)nullptr, pm, (S*)pool, 0));
  } else {
    RC(launch_seg<k_prep_prove<C>>(c, "k_prep_prove", 1, 64, (size_t)1, m, n, kx, ky, (const S*)dG, (const S*)dR,
              (const S*)dR, (const S*)dR, (const S*)nullptr, (const S*)nullptr, (const S*)nullptr, (const S*)nullptr, pm,
              (S*)pool, 0));
  }
  size_t cnt = (size_t)rows * cols;
  RC(launch(c, "k_fr_to_mont", k_fr_to_mont<C>, cnt, 64, cnt, (const S*)pool + pm.PSI, (S*)dout));
  return st.back(out, dout, cnt * sizeof(S));
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
// ---- wire format (gs_wire.cuh): arrays of elements, host pointers -------------------------------------
template <class C> struct WireImpl {
  typedef Fq<C> F1;
  typedef Fp2<C> F2;
  template <class F> static int enc_pts(gs_ctx* c, size_t n, int compressed, const void* pts, uint8_t* out) {
    if (n == 0) return GS_OK;
    size_t pb = AFFB(C, F), wb = wire_point_bytes<C, F>(compressed != 0);
    return staged_call(c, {{pts, n * pb}}, {{out, n * wb}}, [&](void** d) {
      return launch(c, "k_wire_enc_pts", k_wire_enc_pts<C, F>, n, 64, n, (const uint8_t*)d[0], compressed, (uint8_t*)d[1]);
    });
  }
  template <class F>
  static int dec_pts(gs_ctx* c, size_t n, int compressed, int validate, const uint8_t* in, void* pts, uint8_t* ok) {
    if (n == 0) return GS_OK;
    size_t pb = AFFB(C, F), wb = wire_point_bytes<C, F>(compressed != 0);
    return staged_call(c, {{in, n * wb}}, {{pts, n * pb}, {ok, n}}, [&](void** d) {
      return launch(c, "k_wire_dec_pts", k_wire_dec_pts<C, F>, n, 64, n, (const uint8_t*)d[0], compressed, validate,
                    (uint8_t*)d[1], (uint8_t*)d[2]);
    });
  }
  // on-curve + r-torsion check of in-memory points (device pointers)
  template <class F> static int validate_pts_dev(gs_ctx* c, size_t n, const void* pts, uint8_t* ok) {
    return launch(c, "k_validate_pts", k_validate_pts<C, F>, n, 64, n, (const uint8_t*)pts, ok);
  }
  // what: 0 Fr, 1 GT
  static int fields(gs_ctx* c, int what, int dir, int validate, size_t n, const void* in, void* out, uint8_t* ok) {
    if (n == 0) return GS_OK;
    size_t per = what == 0 ? 1 : 12, eb = what == 0 ? sizeof(Fr<C>) : 4 * C::N, cnt = n * per;
    HostStage st(c);
    void *din, *dout, *dok = nullptr;
    RC(st.in(in, cnt * eb, &din));
    RC(st.out(out, cnt * eb, &dout));
    std::vector<uint8_t> oks(cnt, 1);
    if (dir == 1) RC(st.out(oks.data(), cnt, &dok));
    if (what == 0)
      RC(launch(c, "k_wire_fr", k_wire_fr<C>, cnt, 64, cnt, dir, (const uint8_t*)din, (uint8_t*)dout, (uint8_t*)dok));
    else
      RC(launch(c, "k_wire_fq", k_wire_fq<C>, cnt, 64, cnt, dir, (const uint8_t*)din, (uint8_t*)dout, (uint8_t*)dok));
    RC(st.back(out, dout, cnt * eb));
    if (dir == 1) {
      RC(st.back(oks.data(), dok, cnt));
      for (size_t i = 0; i < n; i++) {
        uint8_t a = 1;
        for (size_t j = 0; j < per; j++) a &= oks[i * per + j];
        ok[i] = a;
      }
      if (what == 1 && validate) {  // PairingOutput validity: f^r = 1
        void* dok2;
        RC(st.in(ok, n, &dok2));
        RC(launch(c, "k_wire_gt_check", k_wire_gt_check<C>, n, 64, n, (const uint8_t*)dout, (uint8_t*)dok2));
        RC(st.back(ok, dok2, n));
      }
      // a rejected element decodes to zero as a whole: k_wire_fq clears only the coefficient that is out of range, and
      // the torsion check runs after the values went back
      for (size_t i = 0; i < n; i++)
        if (!ok[i]) memset((uint8_t*)out + i * per * eb, 0, per * eb);
    }
    return GS_OK;
  }
};

// ---- witness extraction with the binding key (entry points below) ----------------------------------------------------
template <class C> static int set_extraction_key_impl(gs_ctx* c, const void* key) {
  RC(ensure(c, c->xkey, 4 * sizeof(SharedDigits)));
  SharedDigits* sd = (SharedDigits*)c->xkey.p;
  void* stage;
  RC(scratch(c, "xkey.in", 2 * SZ_FR + 4, &stage));
  const Fr<C>* dk = (const Fr<C>*)stage;
  uint8_t* dok = (uint8_t*)stage + 2 * SZ_FR;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(stage, key, 2 * SZ_FR, hipMemcpyHostToDevice));
  int rc = launch(c, "k_extract_key.g1", k_extract_key<C, Fq<C>>, 2, 64, dk, (const uint8_t*)c->tabs->crs_g1.p, sd, dok);
  if (rc == GS_OK)
    rc = launch(c, "k_extract_key.g2", k_extract_key<C, Fp2<C>>, 2, 64, dk + 1, (const uint8_t*)c->tabs->crs_g2.p, sd + 2,
                dok + 2);
  uint8_t ok[4] = {0, 0, 0, 0};
  hipError_t e = hipSuccess;
  if (rc == GS_OK) e = hipMemcpyAsync(ok, dok, 4, hipMemcpyDeviceToHost, c->stream);
  hipMemsetAsync(stage, 0, 2 * SZ_FR, c->stream);  // the staged key goes whatever happened
  hipError_t e2 = hipStreamSynchronize(c->stream);
  if (rc != GS_OK) return rc;
  if (e != hipSuccess || e2 != hipSuccess) return fail(c, GS_ERR_DEVICE, "gs_set_extraction_key", e != hipSuccess ? e : e2);
  static const char* const what[4] = {
      "gs_set_extraction_key: u[0].1 != a1 * u[0].0 (wrong a1)",
      "gs_set_extraction_key: u[1].1 != a1 * u[1].0 (a hiding CRS binds no witness, or wrong a1)",
      "gs_set_extraction_key: v[0].1 != a2 * v[0].0 (wrong a2)",
      "gs_set_extraction_key: v[1].1 != a2 * v[1].0 (a hiding CRS binds no witness, or wrong a2)"};
  for (int i = 0; i < 4; i++)
    if (!ok[i]) return fail(c, GS_ERR_ARG, what[i]);
  c->have_xkey = true;
  return GS_OK;
}
// ---- simulation with the hiding CRS's trapdoor (entry points below) ---------------------------------------------------
// The two checks W1 == t1 u0 and W2 == t2 v0 (W = key[1] + (O, generator), derived at gs_set_crs), then the context's
// copy of t1, t2.  The staged copy goes whatever happened; a refused key is wiped by the caller (clear_simulation_key).
template <class C> static int set_simulation_key_impl(gs_ctx* c, const void* key) {
  RC(ensure(c, c->skey, 2 * SZ_FR));
  void* stage;
  RC(scratch(c, "skey.in", 2 * SZ_FR + 4, &stage));
  const Fr<C>* dk = (const Fr<C>*)stage;
  uint8_t* dok = (uint8_t*)stage + 2 * SZ_FR;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(stage, key, 2 * SZ_FR, hipMemcpyHostToDevice));
  int rc = launch(c, "k_sim_key.g1", k_sim_key<C, Fq<C>>, 2, 64, dk, (const uint8_t*)c->tabs->crs_g1.p, dok);
  if (rc == GS_OK)
    rc = launch(c, "k_sim_key.g2", k_sim_key<C, Fp2<C>>, 2, 64, dk + 1, (const uint8_t*)c->tabs->crs_g2.p, dok + 2);
  uint8_t ok[4] = {0, 0, 0, 0};
  hipError_t e = hipSuccess, e1 = hipSuccess;
  if (rc == GS_OK) e = hipMemcpyAsync(ok, dok, 4, hipMemcpyDeviceToHost, c->stream);
  if (rc == GS_OK) e1 = hipMemcpyAsync(c->skey.p, stage, 2 * SZ_FR, hipMemcpyDeviceToDevice, c->stream);
  hipMemsetAsync(stage, 0, 2 * SZ_FR, c->stream);
  hipError_t e2 = hipStreamSynchronize(c->stream);
  if (rc != GS_OK) return rc;
  if (e != hipSuccess || e1 != hipSuccess || e2 != hipSuccess)
    return fail(c, GS_ERR_DEVICE, "gs_set_simulation_key", e != hipSuccess ? e : e1 != hipSuccess ? e1 : e2);
  static const char* const what[4] = {
      "gs_set_simulation_key: (u[1] + (O, g1)).0 != t1 * u[0].0 (wrong t1)",
      "gs_set_simulation_key: (u[1] + (O, g1)).1 != t1 * u[0].1 (a binding CRS has no trapdoor, or wrong t1)",
      "gs_set_simulation_key: (v[1] + (O, g2)).0 != t2 * v[0].0 (wrong t2)",
      "gs_set_simulation_key: (v[1] + (O, g2)).1 != t2 * v[0].1 (a binding CRS has no trapdoor, or wrong t2)"};
  for (int i = 0; i < 4; i++)
    if (!ok[i]) return fail(c, GS_ERR_ARG, what[i]);
  c->have_skey = true;
  return GS_OK;
}
// ---- randomness drawn on the device (gs_rand.cuh; entry points below) -------------------------------------------------
template <class C>
static int rand_fr_impl(gs_ctx* c, uint32_t domain, uint64_t stream, uint64_t first, size_t count, void* out) {
  return launch(c, "k_rand_fr", k_rand_fr<C>, count, RAND_BLOCK, count, (const uint32_t*)c->rkey.p, domain, stream, first,
                (Fr<C>*)out);
}
template <class C, class F> static int extract_impl(gs_ctx* c, const char* name, int slot, size_t n, const void* coms, void* out) {
  const SharedDigits* sd = (const SharedDigits*)c->xkey.p + slot;
  if (c->endo)
    return launch_seg<k_extract<C, F, true>>(c, name, n, 64, n, (const uint8_t*)coms, sd, (uint8_t*)out);
  return launch_seg<k_extract<C, F, false>>(c, (std::string(name) + ".plain").c_str(), n, 64, n, (const uint8_t*)coms,
                                            sd + 1, (uint8_t*)out);
}

extern "C" {

const char* gs_version(void) { return GS_VERSION; }

int gs_sizes(int curve, size_t out[6]) {
  if (curve != 0 && curve != 1) return GS_ERR_ARG;
  size_t fq = sz_fq(curve);
  out[0] = fq;
  out[1] = SZ_FR;
  out[2] = 2 * fq;
  out[3] = 4 * fq;
  out[4] = 12 * fq;
  out[5] = 2 * 4 * fq + 2 * 8 * fq + 2 * fq + 4 * fq + 12 * fq;
  return GS_OK;
}

int gs_ctx_create(int curve, int device, gs_ctx** out) {
  if (!out || (curve != 0 && curve != 1)) return GS_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return GS_ERR_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return GS_ERR_DEVICE;
  gs_ctx* c = new gs_ctx();
  c->curve = curve;
  c->device = device;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
    c->simd_slots = 4 * (size_t)cus;
  // developer overrides of the planner, documented in include/gs_amd.h next to gs_set_option (which is the API)
  if (const char* e = getenv("GS_COOP_FE")) c->coop_fe = atoi(e);
  if (const char* e = getenv("GS_MILLER_CH")) c->miller_ch = atoi(e);
  if (const char* e = getenv("GS_MILLER_TWIN")) c->miller_twin = atoi(e);
  if (const char* e = getenv("GS_LINE_TABLES")) c->line_tables = atoi(e) != 0;
  if (const char* e = getenv("GS_VAR_TM")) c->var_tm = atoi(e);
  if (const char* e = getenv("GS_VAR_MO")) c->var_mo = atoi(e);
  if (const char* e = getenv("GS_VAR_W")) c->var_w = atoi(e);
  if (const char* e = getenv("GS_RED_K")) c->red_k = atoi(e);
  if (const char* e = getenv("GS_VAR_W2")) c->var_w2 = atoi(e);
  if (const char* e = getenv("GS_ENDO")) c->endo = atoi(e) != 0;
  if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
    delete c;
    return GS_ERR_DEVICE;
  }
  for (int i = 0; i < 3 && c->overlap; i++)
    if (hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking) != hipSuccess) c->overlap = false;
  for (int i = 0; i < 6 && c->overlap; i++)
    if (hipEventCreateWithFlags(&c->sev[i], hipEventDisableTiming) != hipSuccess) c->overlap = false;
  if (!c->overlap) c->side[0] = nullptr;
  if (const char* e = getenv("GS_OVERLAP")) c->overlap = c->overlap && atoi(e) != 0;
  {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    g_ctx_all.push_back(c);
  }
  *out = c;
  return GS_OK;
}

void gs_ctx_destroy(gs_ctx* c) {
  if (!c) return;
  {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    g_ctx_all.erase(std::remove(g_ctx_all.begin(), g_ctx_all.end(), c), g_ctx_all.end());
  }
  hipSetDevice(c->device);
  drain_ctx(c);
  clear_extraction_key(c);
  if (c->xkey.p) hipFree(c->xkey.p);
  clear_simulation_key(c);
  if (c->skey.p) hipFree(c->skey.p);
  clear_rand_key(c);
  if (c->rkey.p) hipFree(c->rkey.p);
  for (auto& t : c->dlog)
    for (DevBuf* b : {&t.slots, &t.aux})
      if (b->p) hipFree(b->p);
  for (void* p : c->deferred_free) hipFree(p);
  if (c->stamp) hipFree(c->stamp);
  for (auto& kv : c->scratch)
    if (kv.second.p) hipFree(kv.second.p);
  for (hipStream_t st : c->side)
    if (st) hipStreamSynchronize(st);
  for (auto& kv : c->plans)
    if (kv.second.dev.p) hipFree(kv.second.dev.p);
  delete c->pool;
  if (c->pin) hipHostFree(c->pin);
  if (c->copy_stream) hipStreamDestroy(c->copy_stream);
  for (hipStream_t st : {c->copy_stream2, c->copy_out_stream, c->copy_out_stream2})
    if (st) hipStreamDestroy(st);
  for (hipEvent_t ev : c->pev)
    if (ev) hipEventDestroy(ev);
  for (hipEvent_t ev : c->pev2)
    if (ev) hipEventDestroy(ev);
  if (c->pev_ready) hipEventDestroy(c->pev_ready);
  c->tabs.reset();  // the CRS tables go with their last context
  for (hipStream_t st : c->side)
    if (st) hipStreamDestroy(st);
  for (hipEvent_t ev : c->sev)
    if (ev) hipEventDestroy(ev);
  if (c->ev0) hipEventDestroy(c->ev0);
  if (c->ev1) hipEventDestroy(c->ev1);
  delete c;
}

int gs_set_stream(gs_ctx* c, void* s) {
  if (!c) return GS_ERR_ARG;
  if ((hipStream_t)s != c->stream) {
    // the named scratch buffers, the side streams and their events are shared by consecutive calls and ordered only
    // through the context's stream: work in flight on the old one finishes before anything goes to the new one
    RC(check_ctx(c, false));
    drain_ctx(c);
  }
  c->stream = (hipStream_t)s;
  return GS_OK;
}
int gs_set_option(gs_ctx* c, const char* key, int value) {
  if (!c || !key) return GS_ERR_ARG;
  std::string k(key);
  if (k == "miller_twin") {
    if (value < -1 || value > 3)
      return fail(c, GS_ERR_ARG, "miller_twin: -1 (planned), 0 single, 1 twin, 2 lane pair (LDS), 3 lane pair (DPP)");
    c->miller_twin = value;
  } else if (k == "var_tab") {
    if (value < -1 || value > 1) return fail(c, GS_ERR_ARG, "var_tab: -1 (planned), 0 Straus lanes, 1 shared per-base window tables");
    c->var_tab = value;
  } else if (k == "var_w2") {
    if (value < -1 || value > 1) return fail(c, GS_ERR_ARG, "var_w2: -1 (planned), 0 one wave per SIMD, 1 two (G1 Straus lanes)");
    c->var_w2 = value;
  } else if (k == "endo") {
    c->endo = value != 0;
  } else if (k == "mixed_merge") {
    if (value < -1 || value > 1) return fail(c, GS_ERR_ARG, "mixed_merge: -1 (planned), 0 parts one after the other, 1 merged launches");
    c->mixed_merge = value;
  } else if (k == "miller_ch") {
    if (value < 0 || value > MILLER_CH) return fail(c, GS_ERR_ARG, "miller_ch: 0 (planned) .. capacity of a Miller lane");
    c->miller_ch = value;
  } else if (k == "var_tm") {
    if (value < 0 || value > 8) return fail(c, GS_ERR_ARG, "var_tm: 0 (planned) .. 8");
    c->var_tm = value;
  } else if (k == "var_mo") {
    if (value != 0 && value != 1 && value != 2 && value != 4) return fail(c, GS_ERR_ARG, "var_mo: 0 (planned), 1, 2, 4");
    c->var_mo = value;
  } else if (k == "var_w") {
    if (value != 0 && value != 4 && value != 5) return fail(c, GS_ERR_ARG, "var_w: 0 (planned), 4, 5");
    c->var_w = value;
  } else if (k == "var_ws_lanes") {
    if (value < 0 || (value > 0 && value < 64) || value % 64) return fail(c, GS_ERR_ARG, "var_ws_lanes: 0 or a multiple of 64");
    c->var_ws_lanes = value;
  } else if (k == "red_k") {
    if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8)
      return fail(c, GS_ERR_ARG, "red_k: 0 (planned), 1, 2, 4, 8");
    c->red_k = value;
  } else if (k == "coop_fe") {
    if (value < 0 || value > 2) return fail(c, GS_ERR_ARG, "coop_fe: 0 never, 1 planned, 2 always");
    c->coop_fe = value;
  } else if (k == "locate_k") {
    if (value != 0 && value != 2 && value != 4 && value != 8) return fail(c, GS_ERR_ARG, "locate_k: 0 (planned), 2, 4, 8");
    c->locate_k = value;
  } else if (k == "eq_pi") {
    if (value < -1 || value > 1) return fail(c, GS_ERR_ARG, "eq_pi: -1 (planned), 0 per-proof pairs, 1 folded in G2");
    c->eq_pi = value;
  } else if (k == "dlog_steps") {
    if (value < 0) return fail(c, GS_ERR_ARG, "dlog_steps: 0 (default) or the giant steps per launch");
    c->dlog_steps = value;
  } else if (k == "dlog_fp_bits") {
    if (value < 0 || value > DLOG_FP_BITS) return fail(c, GS_ERR_ARG, "dlog_fp_bits: 0 (default) or 1 .. 35 fingerprint bits");
    c->dlog_fp_bits = value;
  } else if (k == "line_tables") {
    c->line_tables = value != 0;
  } else if (k == "overlap") {
    c->overlap = value != 0 && c->side[0] != nullptr;
  } else {
    return fail(c, GS_ERR_ARG, "unknown option");
  }
  return GS_OK;
}
int gs_sync(gs_ctx* c) {
  RC(check_ctx(c, false));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // every call joins its side streams into the context's stream before it returns; a call that failed half way may
  // not have, and gs_sync promises the whole context
  for (hipStream_t st : c->side)
    if (st) HIPCHK(c, hipStreamSynchronize(st));
  return GS_OK;
}
const char* gs_last_error(gs_ctx* c) { return c ? c->err.c_str() : "null context"; }

// Page-lock a caller's buffer (a Vec the Rust side reuses from call to call): the host-pointer entry points then move
// it by DMA directly instead of through the staging copy.  The runtime counts registrations of a range silently; the
// library keeps its own list so that a second registration, or the release of an unknown pointer, is an error.
int gs_host_register(gs_ctx* c, void* ptr, size_t bytes) {
  RC(check_ctx(c, false));
  if (!ptr || !bytes) return GS_ERR_ARG;
  std::lock_guard<std::mutex> lk(g_reg_mu);
  if (g_reg.count((const uint8_t*)ptr)) return fail(c, GS_ERR_ARG, "gs_host_register: already registered");
  hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterPortable);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? GS_ERR_ALLOC : GS_ERR_ARG, "hipHostRegister", e);
  }
  g_reg[(const uint8_t*)ptr] = bytes;
  return GS_OK;
}
int gs_host_unregister(gs_ctx* c, void* ptr) {
  RC(check_ctx(c, false));
  if (!ptr) return GS_ERR_ARG;
  std::lock_guard<std::mutex> lk(g_reg_mu);
  if (!g_reg.count((const uint8_t*)ptr)) return fail(c, GS_ERR_ARG, "gs_host_unregister: not registered here");
  // Nothing may still be moving the buffer: the registry is process-wide, so EVERY live context is drained -- its
  // compute stream and its copy queues (a D2H is only gated on the compute stream, not finished with it), the shards
  // of a gs_multi context included (they are contexts of their own on their own devices).
  {
    std::lock_guard<std::mutex> lk2(g_ctx_mu);
    for (gs_ctx* o : g_ctx_all) {
      hipSetDevice(o->device);
      drain_ctx(o);
    }
    hipSetDevice(c->device);
  }
  hipError_t e = hipHostUnregister(ptr);
  g_reg.erase((const uint8_t*)ptr);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, GS_ERR_ARG, "hipHostUnregister", e);
  }
  return GS_OK;
}

// Buffers for a caller that wants the fast path without thinking about it: a mapping of its own
// (anonymous mmap: page-aligned, never part of the allocator's heap, so no stale runtime pin can alias it), every page
// touched up front (MAP_POPULATE: no first-touch faults inside a call -- 27-35 ms at 2^16 for result arrays made per
// call), page-locked and entered in the registry: arrays inside it go by DMA straight from / to the caller's memory.
static std::mutex g_alloc_mu;
static std::map<void*, size_t> g_alloc;  // gs_host_alloc: start -> mapped bytes
int gs_host_alloc(gs_ctx* c, size_t bytes, void** out) {
  RC(check_ctx(c, false));
  if (!out || !bytes) return GS_ERR_ARG;
  *out = nullptr;
  const size_t page = 4096, len = (bytes + page - 1) / page * page;
  void* p = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_POPULATE, -1, 0);
  if (p == MAP_FAILED) return fail(c, GS_ERR_ALLOC, "gs_host_alloc: mmap");
  int rc = gs_host_register(c, p, len);
  if (rc != GS_OK) {
    munmap(p, len);
    return rc;
  }
  {
    std::lock_guard<std::mutex> lk(g_alloc_mu);
    g_alloc[p] = len;
  }
  *out = p;
  return GS_OK;
}
int gs_host_free(gs_ctx* c, void* ptr) {
  RC(check_ctx(c, false));
  if (!ptr) return GS_ERR_ARG;
  size_t len = 0;
  {
    std::lock_guard<std::mutex> lk(g_alloc_mu);
    auto it = g_alloc.find(ptr);
    if (it == g_alloc.end()) return fail(c, GS_ERR_ARG, "gs_host_free: not a gs_host_alloc buffer");
    len = it->second;
    g_alloc.erase(it);
  }
  int rc = gs_host_unregister(c, ptr);  // drains every context first
  munmap(ptr, len);
  return rc;
}

int gs_set_crs(gs_ctx* c, const void* crs) {
  RC(check_ctx(c, false));
  if (!crs) return GS_ERR_ARG;
  drain_ctx(c);  // kernels in flight read the tables this call may free (their last reference can be this context's)
  clear_extraction_key(c);  // a key belongs to the CRS it was checked against
  clear_simulation_key(c);
  return DISPATCH(c, set_crs(c, crs));
}

// ---- CRS generation (generator.rs:81-118) --------------------------------------------
int gs_crs_generate(gs_ctx* c, const void* p1, const void* p2, const void* sc, void* out) {
  RC(check_ctx(c, false));
  if (!p1 || !p2 || !sc || !out) return fail(c, GS_ERR_ARG, "null pointer");
  size_t fq = sz_fq(c->curve), g1 = 2 * fq, g2 = 4 * fq;
  const uint8_t* s = (const uint8_t*)sc;  // a1, a2, t1, t2
  uint8_t* o = (uint8_t*)out;
  std::vector<uint8_t> q1(g1), u1(g1), v1(g1), q2(g2), u2(g2), v2(g2);
  // q = a*p, u = t*p, v = t*q   (prepare_real_binding_key: v = q.mul(t) - 0)
  RC(gs_g1_mul_batch(c, 1, p1, 1, s + 0 * SZ_FR, q1.data()));
  RC(gs_g1_mul_batch(c, 1, p1, 1, s + 2 * SZ_FR, u1.data()));
  RC(gs_g1_mul_batch(c, 1, q1.data(), 1, s + 2 * SZ_FR, v1.data()));
  RC(gs_g2_mul_batch(c, 1, p2, 1, s + 1 * SZ_FR, q2.data()));
  RC(gs_g2_mul_batch(c, 1, p2, 1, s + 3 * SZ_FR, u2.data()));
  RC(gs_g2_mul_batch(c, 1, q2.data(), 1, s + 3 * SZ_FR, v2.data()));
  memcpy(o, p1, g1); o += g1;
  memcpy(o, q1.data(), g1); o += g1;
  memcpy(o, u1.data(), g1); o += g1;
  memcpy(o, v1.data(), g1); o += g1;
  memcpy(o, p2, g2); o += g2;
  memcpy(o, q2.data(), g2); o += g2;
  memcpy(o, u2.data(), g2); o += g2;
  memcpy(o, v2.data(), g2); o += g2;
  memcpy(o, p1, g1); o += g1;
  memcpy(o, p2, g2); o += g2;
  return gs_multi_pairing_batch(c, 1, 1, p1, p2, o);
}

// The simulation ("hiding") key of generator.rs:65-77: identical except v = t*q - generator, so that commitments are
// perfectly hiding.  t*q - p is one left_mul with the row (t, -1) over the column ((q, q), (p, p)).
int gs_crs_generate_hiding(gs_ctx* c, const void* p1, const void* p2, const void* sc, void* out) {
  RC(gs_crs_generate(c, p1, p2, sc, out));
  size_t fq = sz_fq(c->curve), g1 = 2 * fq, g2 = 4 * fq;
  const uint8_t* s = (const uint8_t*)sc;
  uint8_t* o = (uint8_t*)out;
  // Montgomery form of -1: r - (2^256 mod r)
  uint32_t m1[8];
  {
    uint64_t br = 0;
    for (int i = 0; i < 8; i++) {
      uint32_t rw = c->curve == 0 ? Bls12_381::R_WORDS[i] : Bn254::R_WORDS[i];
      uint32_t ow = c->curve == 0 ? Bls12_381::Q_ONE[i] : Bn254::Q_ONE[i];
      uint64_t x = (uint64_t)rw - ow - br;
      m1[i] = (uint32_t)x;
      br = (x >> 63) & 1;
    }
  }
  std::vector<uint8_t> lhs(2 * SZ_FR), col, res;
  memcpy(lhs.data() + SZ_FR, m1, SZ_FR);
  // G1: out layout u0 = (p1, q1), u1 = (t1 p1, v1)
  memcpy(lhs.data(), s + 2 * SZ_FR, SZ_FR);
  col.assign(4 * g1, 0);
  res.assign(2 * g1, 0);
  memcpy(col.data(), o + g1, g1);           // (q1, q1)
  memcpy(col.data() + g1, o + g1, g1);
  memcpy(col.data() + 2 * g1, p1, g1);      // (p1, p1)
  memcpy(col.data() + 3 * g1, p1, g1);
  RC(gs_mat_left_mul_com1(c, 1, 2, lhs.data(), col.data(), res.data()));
  memcpy(o + 3 * g1, res.data(), g1);
  // G2: v0 = (p2, q2), v1 = (t2 p2, v2) after the 4 G1 points
  uint8_t* o2 = o + 4 * g1;
  memcpy(lhs.data(), s + 3 * SZ_FR, SZ_FR);
  col.assign(4 * g2, 0);
  res.assign(2 * g2, 0);
  memcpy(col.data(), o2 + g2, g2);
  memcpy(col.data() + g2, o2 + g2, g2);
  memcpy(col.data() + 2 * g2, p2, g2);
  memcpy(col.data() + 3 * g2, p2, g2);
  RC(gs_mat_left_mul_com2(c, 1, 2, lhs.data(), col.data(), res.data()));
  memcpy(o2 + 3 * g2, res.data(), g2);
  return GS_OK;
}

// ---- commit ------------------------------------------------------------------
#define COMMIT_DEV(NAME, FT, GROUP, TAB, TAG)                                                              \
  int NAME(gs_ctx* c, size_t n, const void* v, const void* r, void* out) {                                 \
    RC(check_ctx(c, true));                                                                                \
    if (n == 0) return GS_OK;                                                                              \
    if (!v || !r || !out) return GS_ERR_ARG;                                                               \
    if (c->curve == 0)                                                                                     \
      return Impl<Bls12_381>::commit<FT<Bls12_381>>(c, n, GROUP, v, r, out, (const Aff<FT<Bls12_381>>*)c->tabs->TAB.p, TAG); \
    return Impl<Bn254>::commit<FT<Bn254>>(c, n, GROUP, v, r, out, (const Aff<FT<Bn254>>*)c->tabs->TAB.p, TAG);   \
  }
COMMIT_DEV(gs_commit_g1_dev, Fq, true, tab16_g1, ".cg1")
COMMIT_DEV(gs_commit_g2_dev, Fp2, true, tab16_g2, ".cg2")
COMMIT_DEV(gs_commit_fr_b1_dev, Fq, false, tab16_g1, ".cg1")
COMMIT_DEV(gs_commit_fr_b2_dev, Fp2, false, tab16_g2, ".cg2")

// vq: Fq per committed value (0: an Fr scalar), kc: scalars of randomness per value, oq: Fq per commitment
static int commit_host(gs_ctx* c, int (*dev)(gs_ctx*, size_t, const void*, const void*, void*), size_t vq, size_t kc,
                       size_t oq, size_t n, const void* v, const void* r, void* out) {
  RC(check_ctx(c, true));
  if (n == 0) return GS_OK;
  if (!v || !r || !out) return GS_ERR_ARG;
  const size_t fq = sz_fq(c->curve);
  return staged_call(c, {{v, n * (vq ? vq * fq : SZ_FR)}, {r, n * kc * SZ_FR}}, {{out, n * oq * fq}},
                     [&](void** d) { return dev(c, n, d[0], d[1], d[2]); });
}
int gs_commit_g1(gs_ctx* c, size_t n, const void* v, const void* r, void* out) {
  return commit_host(c, gs_commit_g1_dev, 2, 2, 4, n, v, r, out);
}
int gs_commit_g2(gs_ctx* c, size_t n, const void* v, const void* r, void* out) {
  return commit_host(c, gs_commit_g2_dev, 4, 2, 8, n, v, r, out);
}
int gs_commit_fr_b1(gs_ctx* c, size_t n, const void* v, const void* r, void* out) {
  return commit_host(c, gs_commit_fr_b1_dev, 0, 1, 4, n, v, r, out);
}
int gs_commit_fr_b2(gs_ctx* c, size_t n, const void* v, const void* r, void* out) {
  return commit_host(c, gs_commit_fr_b2_dev, 0, 1, 8, n, v, r, out);
}

// ---- prove / verify / rerandomize: shared plumbing ------------------------------------------------------------
static int check_shape(gs_ctx* c, int ty, int m, int n) {
  if (ty < 0 || ty > 3) return fail(c, GS_ERR_ARG, "bad equation type");
  // the reference indexes rand[0] / gamma[0]: empty variable lists panic (prove.rs:106-113)
  if (m < 1 || n < 1) return fail(c, GS_ERR_SHAPE, "m and n must be >= 1 (reference asserts, prove.rs:106-113)");
  if (!lay::shape_fits(m, n)) return fail(c, GS_ERR_SHAPE, "shape too large for task tables");
  return GS_OK;
}

// One homogeneous batch of any of the three operations.  p[] is indexed by the operation's HostPipe slot (PI_* / VI_*
// / RI_*): host pointers at the un-suffixed entry points, device pointers at the _dev ones and inside.
struct BatchArgs {
  int ty;
  size_t N;
  int m, n;
  bool shared;  // a Statement('s part): ONE copy of X, Y, R, S and of the commitments for all N equations
  const void* p[14];
  uint64_t stream = 0;  // the drawn entries: the generator's stream number of this call
  void* out(int slot) const { return const_cast<void*>(p[slot]); }
};
// An operation states its arrays ONCE: HostPipe slot (= index into BatchArgs::p), which entry of the layout table
// gives its bytes, direction, and whether the pointer may be NULL.  The null check, the staging of a host-pointer call
// and the overlap check all walk this list.
enum { ARR_IN = 0, ARR_OUT = 1, ARR_OPT = 2 };
struct ArrDesc {
  int slot;
  lay::Array arr;
  int flags;
};
struct Op {
  const ArrDesc* arrs;
  int narrs;
  const int* (*order)(int ty);  // host-pointer calls: the order in which the inputs are staged
  int norder;
  int (*run)(gs_ctx*, const BatchArgs&);  // the kernels of a checked, non-empty batch (device pointers)
};
static lay::Layout layout_of(const gs_ctx* c, const BatchArgs& a) {
  return lay::Layout(sz_fq(c->curve), a.ty, a.N, a.m, a.n, a.shared);
}
static int batch_check(gs_ctx* c, const Op& op, const BatchArgs& a) {
  RC(check_ctx(c, true));
  RC(check_shape(c, a.ty, a.m, a.n));
  if (a.N == 0) return GS_OK;
  for (int i = 0; i < op.narrs; i++)
    if (!(op.arrs[i].flags & ARR_OPT) && !a.p[op.arrs[i].slot]) return fail(c, GS_ERR_ARG, "null pointer");
  return GS_OK;
}
static int batch_dev(gs_ctx* c, const Op& op, const BatchArgs& a) {
  RC(batch_check(c, op, a));
  return a.N == 0 ? (int)GS_OK : op.run(c, a);
}
// A host-pointer call runs in three phases so that a mixed call can interleave several sub-batches: stage (the arrays
// are declared, the workers start copying), run (kernels enqueued behind per-array upload events), HostPipe::finish
// (outputs back, stream drained).
static int batch_stage(gs_ctx* c, const Op& op, const BatchArgs& a, HostPipe& hp, size_t base, bool start) {
  const lay::Layout L = layout_of(c, a);
  for (int i = 0; i < op.narrs; i++) {
    const ArrDesc& d = op.arrs[i];
    if (d.flags & ARR_OUT)
      hp.out(d.slot, a.out(d.slot), L.bytes[d.arr]);
    else
      hp.in(d.slot, a.p[d.slot], L.bytes[d.arr]);
  }
  return start ? hp.begin(op.order(a.ty), op.norder, base, base == 0) : (int)GS_OK;
}
static int batch_run_staged(gs_ctx* c, const Op& op, const BatchArgs& a, const HostPipe& hp) {
  BatchArgs d = a;
  for (int i = 0; i < op.narrs; i++) d.p[op.arrs[i].slot] = hp.dev(op.arrs[i].slot);
  return op.run(c, d);
}
static int batch_host_checked(gs_ctx* c, const Op& op, const BatchArgs& a) {
  HostPipe hp(c);
  RC(batch_stage(c, op, a, hp, 0, true));
  RC(batch_run_staged(c, op, a, hp));
  return hp.finish();
}
static int batch_host(gs_ctx* c, const Op& op, const BatchArgs& a) {
  RC(batch_check(c, op, a));
  return a.N == 0 ? (int)GS_OK : batch_host_checked(c, op, a);
}

// ---- prove -------------------------------------------------------------------
static const ArrDesc kProveArrs[] = {
    {PI_X, lay::X, ARR_IN},      {PI_Y, lay::Y, ARR_IN},      {PI_A, lay::A, ARR_IN},
    {PI_B, lay::B, ARR_IN},      {PI_G, lay::GAMMA, ARR_IN},  {PI_R, lay::R, ARR_IN},
    {PI_S, lay::S, ARR_IN},      {PI_T, lay::T, ARR_IN},      {PO_XC, lay::XCOMS, ARR_OUT | ARR_OPT},
    {PO_YC, lay::YCOMS, ARR_OUT | ARR_OPT}, {PO_PI, lay::PI, ARR_OUT}, {PO_TH, lay::THETA, ARR_OUT}};
static const int* prove_order(int) {
  // staging order = the order prove() asks for them (scalars, then the G2 side's arguments, then the G1 side's)
  static const int order[] = {PI_G, PI_R, PI_S, PI_T, PI_Y, PI_B, PI_X, PI_A};  // (Y before B: the fixed-base kernel reads Y)
  return order;
}
static int prove_run(gs_ctx* c, const BatchArgs& a) {
  const void* const* p = a.p;
  void *xcoms = a.out(PO_XC), *ycoms = a.out(PO_YC);
  if (a.shared) {
    // a Statement: the commitments, once (commit.rs:78-100,125-156,178-200,225-256); the prover then writes none
    RC(need(c, BIT(PI_X) | BIT(PI_Y) | BIT(PI_R) | BIT(PI_S)));
    if (xcoms) RC((lay::x_is_group(a.ty) ? gs_commit_g1_dev : gs_commit_fr_b1_dev)(c, (size_t)a.m, p[PI_X], p[PI_R], xcoms));
    if (ycoms) RC((lay::y_is_group(a.ty) ? gs_commit_g2_dev : gs_commit_fr_b2_dev)(c, (size_t)a.n, p[PI_Y], p[PI_S], ycoms));
    xcoms = ycoms = nullptr;
  }
  return DISPATCH(c, prove(c, a.ty, a.N, a.m, a.n, p[PI_X], p[PI_Y], p[PI_A], p[PI_B], p[PI_G], p[PI_R], p[PI_S],
                           p[PI_T], xcoms, ycoms, a.out(PO_PI), a.out(PO_TH), a.shared));
}
static const Op kProve = {kProveArrs, sizeof kProveArrs / sizeof *kProveArrs, prove_order, 8, prove_run};
static BatchArgs from_part(const gs_prove_part& p) {
  return BatchArgs{p.equ_type, p.N, p.m, p.n, p.shared_vars != 0,
                   {p.X, p.Y, p.A, p.B, p.Gamma, p.R, p.S, p.T, p.xcoms, p.ycoms, p.pi, p.theta}};
}
int gs_prove_batch_dev(gs_ctx* c, int ty, size_t N, int m, int n, const void* X, const void* Y, const void* A,
                       const void* B, const void* G, const void* R, const void* S, const void* T, void* xcoms,
                       void* ycoms, void* pi, void* theta) {
  return batch_dev(c, kProve, {ty, N, m, n, false, {X, Y, A, B, G, R, S, T, xcoms, ycoms, pi, theta}});
}
int gs_prove_batch(gs_ctx* c, int ty, size_t N, int m, int n, const void* X, const void* Y, const void* A,
                   const void* B, const void* G, const void* R, const void* S, const void* T, void* xcoms,
                   void* ycoms, void* pi, void* theta) {
  return batch_host(c, kProve, {ty, N, m, n, false, {X, Y, A, B, G, R, S, T, xcoms, ycoms, pi, theta}});
}
// Statement: E equations of one type over the SAME committed variables (statement.rs:24-28,109)
int gs_prove_statement_dev(gs_ctx* c, int ty, size_t E, int m, int n, const void* X, const void* Y, const void* A,
                           const void* B, const void* G, const void* R, const void* S, const void* T, void* xcoms,
                           void* ycoms, void* pi, void* theta) {
  return batch_dev(c, kProve, {ty, E, m, n, true, {X, Y, A, B, G, R, S, T, xcoms, ycoms, pi, theta}});
}
int gs_prove_statement(gs_ctx* c, int ty, size_t E, int m, int n, const void* X, const void* Y, const void* A,
                       const void* B, const void* G, const void* R, const void* S, const void* T, void* xcoms,
                       void* ycoms, void* pi, void* theta) {
  return batch_host(c, kProve, {ty, E, m, n, true, {X, Y, A, B, G, R, S, T, xcoms, ycoms, pi, theta}});
}

// ---- verify ------------------------------------------------------------------
static const ArrDesc kVerifyArrs[] = {
    {VI_A, lay::A, ARR_IN},      {VI_B, lay::B, ARR_IN},      {VI_G, lay::GAMMA, ARR_IN},
    {VI_TG, lay::TARGET, ARR_IN}, {VI_XC, lay::XCOMS, ARR_IN}, {VI_YC, lay::YCOMS, ARR_IN},
    {VI_PI, lay::PI, ARR_IN},    {VI_TH, lay::THETA, ARR_IN}, {VO_OK, lay::OK, ARR_OUT}};
static const int* verify_order(int ty) {
  // Gamma and the G1-side arguments first (the verifier's Gamma-MSM runs under the upload of the rest)
  static const int order_g[] = {VI_G, VI_A, VI_XC, VI_TG, VI_B, VI_YC, VI_PI, VI_TH};
  static const int order_s[] = {VI_G, VI_A, VI_B, VI_TG, VI_XC, VI_YC, VI_PI, VI_TH};
  return ty == GS_PPE || ty == GS_MSMEG2 ? order_g : order_s;
}
static int verify_run(gs_ctx* c, const BatchArgs& a) {
  return DISPATCH(c, verify(c, VerifyIn(a.ty, a.N, a.m, a.n, a.p), (uint8_t*)a.out(VO_OK), a.shared));
}
static const Op kVerify = {kVerifyArrs, sizeof kVerifyArrs / sizeof *kVerifyArrs, verify_order, 8, verify_run};
static BatchArgs from_part(const gs_verify_part& p) {
  return BatchArgs{p.equ_type, p.N, p.m, p.n, p.shared_vars != 0,
                   {p.A, p.B, p.Gamma, p.target, p.xcoms, p.ycoms, p.pi, p.theta, p.ok}};
}
int gs_verify_batch_dev(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G,
                        const void* target, const void* xcoms, const void* ycoms, const void* pi, const void* theta,
                        uint8_t* ok) {
  return batch_dev(c, kVerify, {ty, N, m, n, false, {A, B, G, target, xcoms, ycoms, pi, theta, ok}});
}
int gs_verify_batch(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G,
                    const void* target, const void* xcoms, const void* ycoms, const void* pi, const void* theta,
                    uint8_t* ok) {
  return batch_host(c, kVerify, {ty, N, m, n, false, {A, B, G, target, xcoms, ycoms, pi, theta, ok}});
}
int gs_verify_statement_dev(gs_ctx* c, int ty, size_t E, int m, int n, const void* A, const void* B, const void* G,
                            const void* target, const void* xcoms, const void* ycoms, const void* pi,
                            const void* theta, uint8_t* ok) {
  return batch_dev(c, kVerify, {ty, E, m, n, true, {A, B, G, target, xcoms, ycoms, pi, theta, ok}});
}
int gs_verify_statement(gs_ctx* c, int ty, size_t E, int m, int n, const void* A, const void* B, const void* G,
                        const void* target, const void* xcoms, const void* ycoms, const void* pi, const void* theta,
                        uint8_t* ok) {
  return batch_host(c, kVerify, {ty, E, m, n, true, {A, B, G, target, xcoms, ycoms, pi, theta, ok}});
}

// ---- evaluate / check witness: what an equation evaluates to at a witness ------------------------------------------
// One operation behind the eight entries: gs_eval_* pass target_out (EO_T), gs_check_witness_* pass target (EI_TG) and
// ok (EO_OK); the other group stays null.
static const ArrDesc kEvalArrs[] = {
    {EI_X, lay::X, ARR_IN},      {EI_Y, lay::Y, ARR_IN},          {EI_A, lay::A, ARR_IN},
    {EI_B, lay::B, ARR_IN},      {EI_G, lay::GAMMA, ARR_IN},      {EI_TG, lay::TARGET, ARR_IN | ARR_OPT},
    {EO_T, lay::TARGET, ARR_OUT | ARR_OPT}, {EO_OK, lay::OK, ARR_OUT | ARR_OPT}};
static const int* eval_order(int ty) {
  // staging order = the order eval() asks for them: Gamma and the scalar arrays, the G1 arrays, the G2 arrays, the target
  static const int order[4][6] = {{EI_G, EI_A, EI_X, EI_Y, EI_B, EI_TG},
                                  {EI_G, EI_Y, EI_B, EI_X, EI_A, EI_TG},
                                  {EI_G, EI_X, EI_A, EI_Y, EI_B, EI_TG},
                                  {EI_G, EI_X, EI_Y, EI_A, EI_B, EI_TG}};
  return order[ty];
}
static int eval_run(gs_ctx* c, const BatchArgs& a) {
  const void* const* p = a.p;
  return DISPATCH(c, eval(c, a.ty, a.N, a.m, a.n, p[EI_X], p[EI_Y], p[EI_A], p[EI_B], p[EI_G], p[EI_TG], a.out(EO_T),
                          (uint8_t*)a.out(EO_OK), a.shared));
}
static const Op kEval = {kEvalArrs, sizeof kEvalArrs / sizeof *kEvalArrs, eval_order, 6, eval_run};
static BatchArgs eval_args(int ty, size_t N, int m, int n, bool shared, const void* X, const void* Y, const void* A,
                           const void* B, const void* G, const void* target, void* target_out, uint8_t* ok) {
  return BatchArgs{ty, N, m, n, shared, {X, Y, A, B, G, target, target_out, ok}};
}
// check = a gs_check_witness_* entry (target and ok required), else gs_eval_* (target_out required)
static int eval_call(gs_ctx* c, const char* fn, bool host, bool check, const BatchArgs& a) {
  if (c && c->rec) return fail(c, GS_ERR_ARG, (std::string(fn) + " inside a mixed call").c_str());
  RC(batch_check(c, kEval, a));
  if (a.N == 0) return GS_OK;
  if (check ? (!a.p[EI_TG] || !a.p[EO_OK]) : !a.p[EO_T]) return fail(c, GS_ERR_ARG, "null pointer");
  if (!host) return kEval.run(c, a);
  // the output does not alias an input (the staged copy would hide it; the device form reads while it writes)
  const lay::Layout L = layout_of(c, a);
  const ArrDesc& o = kEvalArrs[check ? 7 : 6];
  for (const ArrDesc& i : kEvalArrs) {
    if ((i.flags & ARR_OUT) || !a.p[i.slot]) continue;
    uintptr_t x = (uintptr_t)a.p[o.slot], y = (uintptr_t)a.p[i.slot];
    if (x < y + L.bytes[i.arr] && y < x + L.bytes[o.arr])
      return fail(c, GS_ERR_ARG, (std::string(fn) + ": the output overlaps an input").c_str());
  }
  return batch_host_checked(c, kEval, a);
}
#define GS_EVAL_ENTRY(NAME, HOST, SHARED)                                                                             \
  int NAME(gs_ctx* c, int ty, size_t N, int m, int n, const void* X, const void* Y, const void* A, const void* B,      \
           const void* G, void* target_out) {                                                                          \
    return eval_call(c, #NAME, HOST, false, eval_args(ty, N, m, n, SHARED, X, Y, A, B, G, nullptr, target_out, nullptr)); \
  }
#define GS_CHECK_ENTRY(NAME, HOST, SHARED)                                                                            \
  int NAME(gs_ctx* c, int ty, size_t N, int m, int n, const void* X, const void* Y, const void* A, const void* B,      \
           const void* G, const void* target, uint8_t* ok) {                                                           \
    return eval_call(c, #NAME, HOST, true, eval_args(ty, N, m, n, SHARED, X, Y, A, B, G, target, nullptr, ok));        \
  }
GS_EVAL_ENTRY(gs_eval_batch_dev, false, false)
GS_EVAL_ENTRY(gs_eval_batch, true, false)
GS_EVAL_ENTRY(gs_eval_statement_dev, false, true)
GS_EVAL_ENTRY(gs_eval_statement, true, true)
GS_CHECK_ENTRY(gs_check_witness_batch_dev, false, false)
GS_CHECK_ENTRY(gs_check_witness_batch, true, false)
GS_CHECK_ENTRY(gs_check_witness_statement_dev, false, true)
GS_CHECK_ENTRY(gs_check_witness_statement, true, true)
#undef GS_EVAL_ENTRY
#undef GS_CHECK_ENTRY

// ---- mixed batches: several sub-batches (any types and shapes) in ONE call ----------------------------------------
// configs[2] of the baseline is a batch of PPE, MSMEG1 and MSMEG2 equations; the reference's Statement is a list of
// equations of any type (statement.rs:24-28).  The parts run one after the other on the context's stream.
// Measured and NOT kept (profiles/r3/mixed_streams.txt): one child context per part (own stream, own scratch) so that
// the parts' kernels are in flight together.  These kernels hold one 512-register wave per SIMD and a private segment
// each; dispatches from different queues did not share the chip at all (2^12 mixed: 71.1 ms on three streams, 71.3 ms
// on one), and the extra queues' scratch reservations slowed LATER large batches on the parent fourfold (2^16 PPE
// 320 -> 1400 ms).  What does fill the chip for a mixed batch of a few thousand equations is merging the lanes of
// all parts into single launches (segmented launches, section 4.3 of DESIGN.md).
// Record every part's launches (nothing is enqueued yet), then replay them merged.  A single part simply runs.  The
// kernel profile (gs_prof_enable) times the MERGED launches themselves (go_seg: HIP events around each k_seg launch, under
// the name of its first segment), so that a mixed step's per-kernel times add up to the step that is timed.
// Merged launches pay off while the parts' own launches leave SIMDs idle; from ~2^15 equations on every part fills the
// chip by itself and separate launches with per-part lane shapes are as fast (measured: profiles/r3/mixed_merge.txt).
static bool merge_parts(const gs_ctx* c, size_t total_n) {
  if (c->mixed_merge >= 0) return c->mixed_merge != 0;
  // <= 2^14 equations on a 256-CU device (profiles/r3/mixed_merge.txt: merged 103 against 112 ms in sequence at 2^14,
  // 193 against 182 ms at 2^15, where every part fills the chip with its own lane shapes)
  return total_n <= 16 * c->simd_slots;
}
// buffers parked by ensure() during a recording: the replayed launches may read them, so they go after a stream sync
static int release_deferred(gs_ctx* c, int rc) {
  if (c->deferred_free.empty()) return rc;
  hipStreamSynchronize(c->stream);
  for (void* p : c->deferred_free) hipFree(p);
  c->deferred_free.clear();
  return rc;
}
extern "C++" {
template <class PART> static std::vector<BatchArgs> parts_of(const PART* p, int nparts) {
  std::vector<BatchArgs> a;
  for (int i = 0; i < nparts; i++) a.push_back(from_part(p[i]));
  return a;
}
}  // extern "C++"
static int check_parts(gs_ctx* c, int nparts, const void* p, const char* what) {
  RC(check_ctx(c, true));
  if (nparts < 0 || nparts > GS_MIXED_MAX || (nparts && !p)) return fail(c, GS_ERR_ARG, what);
  return GS_OK;
}
// device pointers: every part is checked as its turn comes (a failed part: nothing was launched when merging)
static int mixed_dev(gs_ctx* c, const Op& op, const std::vector<BatchArgs>& a) {
  const int nparts = (int)a.size();
  size_t total_n = 0;
  for (const BatchArgs& p : a) total_n += p.N;
  if (nparts <= 1 || c->rec || !merge_parts(c, total_n)) {
    for (int i = 0; i < nparts; i++) RC(batch_dev(c, op, a[i]));
    return GS_OK;
  }
  Recorder R;
  R.parts.resize(nparts);
  c->rec = &R;
  c->fill_n = total_n;
  int rc = GS_OK;
  for (int i = 0; i < nparts && rc == GS_OK; i++) {
    R.cur = i;
    c->scratch_tag = i + 1;
    rc = batch_dev(c, op, a[i]);
  }
  c->rec = nullptr;
  c->fill_n = 0;
  c->scratch_tag = 0;
  if (rc == GS_OK) rc = replay(c, R);  // (a failed part: nothing was launched)
  return release_deferred(c, rc);
}
// host pointers: every part is staged into its own region of the pinned buffer (the memcpy workers start at once), the
// parts' launches are recorded behind their upload events and replayed merged, then the outputs come back
static int mixed_host(gs_ctx* c, const Op& op, const std::vector<BatchArgs>& parts, const char* range) {
  std::vector<BatchArgs> a;  // every part's shape and pointers are checked first; empty parts then drop out
  size_t total_n = 0;
  for (const BatchArgs& p : parts) {
    RC(batch_check(c, op, p));
    if (p.N == 0) continue;
    a.push_back(p);
    total_n += p.N;
  }
  RangeGuard rg(range);
  const int np = (int)a.size();
  if (np <= 1 || !merge_parts(c, total_n)) {
    for (int i = 0; i < np; i++) RC(batch_host_checked(c, op, a[i]));
    return GS_OK;
  }
  std::vector<std::unique_ptr<HostPipe>> hp;
  // 1. how much pinned memory the call needs: declare the arrays on throw-away pipes
  size_t need_pin = 0;
  std::vector<size_t> base(np, 0);
  for (int i = 0; i < np; i++) {
    hp.emplace_back(new HostPipe(c));
    base[i] = need_pin;
    need_pin += batch_stage(c, op, a[i], *hp[i], 0, false) == GS_OK ? hp[i]->layout() : 0;
  }
  hp.clear();
  c->pipe = nullptr;
  RC(HostPipe::pin_reserve(c, need_pin));
  // 2. stage for real, every part at its base
  int rc = GS_OK;
  for (int i = 0; i < np && rc == GS_OK; i++) {
    hp.emplace_back(new HostPipe(c));
    c->scratch_tag = i + 1;
    rc = batch_stage(c, op, a[i], *hp[i], base[i], true);
  }
  // 3. record the parts' launches (their need() calls enqueue the uploads and make the stream wait), replay merged
  Recorder R;
  R.parts.resize(np);
  c->rec = &R;
  c->fill_n = total_n;
  for (int i = 0; i < np && rc == GS_OK; i++) {
    R.cur = i;
    c->scratch_tag = i + 1;
    c->pipe = hp[i].get();
    rc = batch_run_staged(c, op, a[i], *hp[i]);
  }
  c->rec = nullptr;
  c->fill_n = 0;
  c->scratch_tag = 0;
  c->pipe = nullptr;
  if (rc == GS_OK) rc = replay(c, R);
  // 4. outputs
  for (int i = 0; i < np; i++) {
    if (rc == GS_OK) {
      c->scratch_tag = i + 1;
      rc = hp[i]->finish();
    }
  }
  c->scratch_tag = 0;
  if (rc != GS_OK) drain_ctx(c);  // uploads / downloads of the parts that did start (not only c->stream)
  return release_deferred(c, rc);
}
int gs_prove_mixed_dev(gs_ctx* c, int nparts, const gs_prove_part* p) {
  RC(check_parts(c, nparts, p, "gs_prove_mixed: 0..8 parts"));
  RangeGuard rg("gs.prove_mixed");
  return mixed_dev(c, kProve, parts_of(p, nparts));
}
int gs_verify_mixed_dev(gs_ctx* c, int nparts, const gs_verify_part* p) {
  RC(check_parts(c, nparts, p, "gs_verify_mixed: 0..8 parts"));
  RangeGuard rg("gs.verify_mixed");
  return mixed_dev(c, kVerify, parts_of(p, nparts));
}
int gs_prove_mixed(gs_ctx* c, int nparts, const gs_prove_part* p) {
  RC(check_parts(c, nparts, p, "gs_prove_mixed: 0..8 parts"));
  return mixed_host(c, kProve, parts_of(p, nparts), "gs.prove_mixed");
}
int gs_verify_mixed(gs_ctx* c, int nparts, const gs_verify_part* p) {
  RC(check_parts(c, nparts, p, "gs_verify_mixed: 0..8 parts"));
  return mixed_host(c, kVerify, parts_of(p, nparts), "gs.verify_mixed");
}

// ---- rerandomize: fresh commitments and proofs from old ones, without the witness -----------------------------
static const ArrDesc kRerandArrs[] = {
    {RI_A, lay::A, ARR_IN},       {RI_B, lay::B, ARR_IN},       {RI_G, lay::GAMMA, ARR_IN}, {RI_R, lay::R, ARR_IN},
    {RI_S, lay::S, ARR_IN},       {RI_T, lay::T, ARR_IN},       {RI_XC, lay::XCOMS, ARR_IN}, {RI_YC, lay::YCOMS, ARR_IN},
    {RI_PI, lay::PI, ARR_IN},     {RI_TH, lay::THETA, ARR_IN},  {RO_XC, lay::XCOMS, ARR_OUT}, {RO_YC, lay::YCOMS, ARR_OUT},
    {RO_PI, lay::PI, ARR_OUT},    {RO_TH, lay::THETA, ARR_OUT}};
static const int* rerand_order(int) {
  // staging order = the order rerandomize() asks for them: scalars, then the G2 side's arrays, then the G1 side's
  static const int order[] = {RI_G, RI_R, RI_S, RI_T, RI_B, RI_A, RI_YC, RI_PI, RI_XC, RI_TH};
  return order;
}
static int rerand_run(gs_ctx* c, const BatchArgs& a) {
  const void* const* p = a.p;
  return DISPATCH(c, rerandomize(c, a.ty, a.N, a.m, a.n, p[RI_A], p[RI_B], p[RI_G], p[RI_XC], p[RI_YC], p[RI_PI],
                                 p[RI_TH], p[RI_R], p[RI_S], p[RI_T], a.out(RO_XC), a.out(RO_YC), a.out(RO_PI),
                                 a.out(RO_TH), a.shared));
}
static const Op kRerand = {kRerandArrs, sizeof kRerandArrs / sizeof *kRerandArrs, rerand_order, 10, rerand_run};
// the arguments in the order of the public signatures -> slot order (the scalars R', S', T' come before the old
// commitments and proofs there)
static_assert(RI_R == 3 && RI_XC == 6 && RO_XC == 10 && RO_TH == 13, "rerand_args lists its pointers in slot order");
static BatchArgs rerand_args(int ty, size_t N, int m, int n, bool shared, const void* A, const void* B, const void* G,
                             const void* xc, const void* yc, const void* pi, const void* th, const void* R, const void* S,
                             const void* T, void* xco, void* yco, void* pio, void* tho) {
  return BatchArgs{ty, N, m, n, shared, {A, B, G, R, S, T, xc, yc, pi, th, xco, yco, pio, tho}};
}
static int rerand_host(gs_ctx* c, const BatchArgs& a) {
  RC(batch_check(c, kRerand, a));
  if (a.N == 0) return GS_OK;
  // outputs do not alias inputs or each other (the device reads old commitments after it has written new ones)
  const lay::Layout L = layout_of(c, a);
  for (const ArrDesc& o : kRerandArrs) {
    if (!(o.flags & ARR_OUT)) continue;
    for (const ArrDesc& i : kRerandArrs) {
      if (i.slot == o.slot) continue;
      uintptr_t x = (uintptr_t)a.p[o.slot], y = (uintptr_t)a.p[i.slot];
      if (x < y + L.bytes[i.arr] && y < x + L.bytes[o.arr])
        return fail(c, GS_ERR_ARG, "rerandomize: an output overlaps another array");
    }
  }
  return batch_host_checked(c, kRerand, a);
}
int gs_rerandomize_batch_dev(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G,
                             const void* xcoms, const void* ycoms, const void* pi, const void* theta, const void* R,
                             const void* S, const void* T, void* xcoms_out, void* ycoms_out, void* pi_out,
                             void* theta_out) {
  return batch_dev(c, kRerand, rerand_args(ty, N, m, n, false, A, B, G, xcoms, ycoms, pi, theta, R, S, T, xcoms_out,
                                           ycoms_out, pi_out, theta_out));
}
int gs_rerandomize_batch(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G,
                         const void* xcoms, const void* ycoms, const void* pi, const void* theta, const void* R,
                         const void* S, const void* T, void* xcoms_out, void* ycoms_out, void* pi_out, void* theta_out) {
  return rerand_host(c, rerand_args(ty, N, m, n, false, A, B, G, xcoms, ycoms, pi, theta, R, S, T, xcoms_out, ycoms_out,
                                    pi_out, theta_out));
}
int gs_rerandomize_statement_dev(gs_ctx* c, int ty, size_t E, int m, int n, const void* A, const void* B, const void* G,
                                 const void* xcoms, const void* ycoms, const void* pi, const void* theta, const void* R,
                                 const void* S, const void* T, void* xcoms_out, void* ycoms_out, void* pi_out,
                                 void* theta_out) {
  return batch_dev(c, kRerand, rerand_args(ty, E, m, n, true, A, B, G, xcoms, ycoms, pi, theta, R, S, T, xcoms_out,
                                           ycoms_out, pi_out, theta_out));
}
int gs_rerandomize_statement(gs_ctx* c, int ty, size_t E, int m, int n, const void* A, const void* B, const void* G,
                             const void* xcoms, const void* ycoms, const void* pi, const void* theta, const void* R,
                             const void* S, const void* T, void* xcoms_out, void* ycoms_out, void* pi_out,
                             void* theta_out) {
  return rerand_host(c, rerand_args(ty, E, m, n, true, A, B, G, xcoms, ycoms, pi, theta, R, S, T, xcoms_out, ycoms_out,
                                    pi_out, theta_out));
}

// ---- simulate: commitments and proofs from the hiding CRS's trapdoor, without any witness ---------------------------
static const ArrDesc kSimulateArrs[] = {
    {SI_A, lay::A, ARR_IN},       {SI_B, lay::B, ARR_IN},       {SI_G, lay::GAMMA, ARR_IN}, {SI_TG, lay::TARGET, ARR_IN},
    {SI_R, lay::R, ARR_IN},       {SI_S, lay::S, ARR_IN},       {SI_T, lay::T, ARR_IN},
    {SO_XC, lay::XCOMS, ARR_OUT | ARR_OPT}, {SO_YC, lay::YCOMS, ARR_OUT | ARR_OPT}, {SO_PI, lay::PI, ARR_OUT},
    {SO_TH, lay::THETA, ARR_OUT}};
static const int* simulate_order(int) {
  // staging order = the order simulate() asks for them: the scalars, then the G1 side's points, then the G2 side's
  // (of A, B, target the scalar-valued ones are read by the preparation kernel; they are small)
  static const int order[] = {SI_G, SI_R, SI_S, SI_T, SI_TG, SI_A, SI_B};
  return order;
}
static int simulate_run(gs_ctx* c, const BatchArgs& a) {
  const void* const* p = a.p;
  return DISPATCH(c, simulate(c, a.ty, a.N, a.m, a.n, p[SI_A], p[SI_B], p[SI_G], p[SI_TG], p[SI_R], p[SI_S], p[SI_T],
                              a.out(SO_XC), a.out(SO_YC), a.out(SO_PI), a.out(SO_TH), a.shared));
}
static const Op kSimulate = {kSimulateArrs, sizeof kSimulateArrs / sizeof *kSimulateArrs, simulate_order, 7, simulate_run};
static int simulate_call(gs_ctx* c, const char* fn, bool host, const BatchArgs& a) {
  if (c && c->rec) return fail(c, GS_ERR_ARG, (std::string(fn) + " inside a mixed call").c_str());
  RC(batch_check(c, kSimulate, a));
  if (!c->have_skey) return fail(c, GS_ERR_ARG, (std::string(fn) + ": gs_set_simulation_key has not been called").c_str());
  if (a.ty == GS_PPE)
    return fail(c, GS_ERR_ARG,
                (std::string(fn) + ": GS_PPE is refused -- iota_T(t) of a general target t in GT has no preimage the "
                                   "simulator could pair its way to, and a PPE with target one is already simulated by "
                                   "gs_prove_batch at the identity witness").c_str());
  if (a.N == 0) return GS_OK;
  if (!host) return kSimulate.run(c, a);
  // outputs do not alias inputs or each other (the staged copies would hide it; the device form's contract)
  const lay::Layout L = layout_of(c, a);
  for (const ArrDesc& o : kSimulateArrs) {
    if (!(o.flags & ARR_OUT) || !a.p[o.slot]) continue;
    for (const ArrDesc& i : kSimulateArrs) {
      if (i.slot == o.slot || !a.p[i.slot]) continue;
      uintptr_t x = (uintptr_t)a.p[o.slot], y = (uintptr_t)a.p[i.slot];
      if (x < y + L.bytes[i.arr] && y < x + L.bytes[o.arr])
        return fail(c, GS_ERR_ARG, (std::string(fn) + ": an output overlaps another array").c_str());
    }
  }
  return batch_host_checked(c, kSimulate, a);
}
#define GS_SIMULATE_ENTRY(NAME, HOST, SHARED)                                                                        \
  int NAME(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G, const void* target, \
           const void* Rc, const void* Sc, const void* Tf, void* xcoms, void* ycoms, void* pi, void* theta) {         \
    return simulate_call(c, #NAME, HOST,                                                                             \
                         BatchArgs{ty, N, m, n, SHARED, {A, B, G, target, Rc, Sc, Tf, xcoms, ycoms, pi, theta}});     \
  }
GS_SIMULATE_ENTRY(gs_simulate_batch_dev, false, false)
GS_SIMULATE_ENTRY(gs_simulate_batch, true, false)
GS_SIMULATE_ENTRY(gs_simulate_statement_dev, false, true)
GS_SIMULATE_ENTRY(gs_simulate_statement, true, true)
#undef GS_SIMULATE_ENTRY
int gs_set_simulation_key(gs_ctx* c, const void* t1t2) {
  RC(check_ctx(c, false));
  clear_simulation_key(c);
  if (!t1t2) return GS_OK;
  RC(check_ctx(c, true));
  if (c->rec) return fail(c, GS_ERR_ARG, "gs_set_simulation_key inside a mixed call");
  int rc = DISPATCH_FN(c, set_simulation_key_impl, (c, t1t2));
  if (rc != GS_OK) clear_simulation_key(c);  // a refused key leaves nothing behind
  return rc;
}

// ---- randomness drawn on the device: the keyed ChaCha20 of gs_rand.cuh ------------------------------------------------
int gs_rand_set_key(gs_ctx* c, const void* key32) {
  RC(check_ctx(c, false));
  if (c->rec) return fail(c, GS_ERR_ARG, "gs_rand_set_key inside a mixed call");
  clear_rand_key(c);
  if (!key32) return GS_OK;
  RC(ensure(c, c->rkey, 32));
  // Straight from the caller's buffer into the context's copy: the library keeps no staged copy of this key.  The
  // stream is drained first (draws under the old key, the memset above) and the copy is complete on return.
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(c->rkey.p, key32, 32, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    clear_rand_key(c);  // (rkey.p is set: whatever arrived is zeroed)
    return fail(c, GS_ERR_DEVICE, "gs_rand_set_key", e);
  }
  c->have_rkey = true;
  return GS_OK;
}
static const uint64_t RAND_COUNTERS = (uint64_t)1 << 32;  // block counters of one (domain, stream): the counter never wraps
static int rand_check(gs_ctx* c, const char* fn) {
  RC(check_ctx(c, false));
  if (c->rec) return fail(c, GS_ERR_ARG, (std::string(fn) + " inside a mixed call").c_str());
  if (!c->have_rkey) return fail(c, GS_ERR_ARG, (std::string(fn) + ": gs_rand_set_key has not been called").c_str());
  return GS_OK;
}
// count Fr of (domain, stream) from element `first` into device memory, on the current stream
static int rand_fr_launch(gs_ctx* c, uint32_t domain, uint64_t stream, uint64_t first, size_t count, void* out) {
  if (first > RAND_COUNTERS || (uint64_t)count > RAND_COUNTERS - first)
    return fail(c, GS_ERR_SHAPE, "gs_rand_fr: first + count > 2^32 (one block per scalar, 32-bit block counter)");
  return DISPATCH_FN(c, rand_fr_impl, (c, domain, stream, first, count, out));
}
static int rand_fr_call(gs_ctx* c, const char* fn, bool host, uint32_t domain, uint64_t stream, uint64_t first,
                        size_t count, void* out) {
  RC(rand_check(c, fn));
  if (first > RAND_COUNTERS || (uint64_t)count > RAND_COUNTERS - first)
    return fail(c, GS_ERR_SHAPE, "gs_rand_fr: first + count > 2^32 (one block per scalar, 32-bit block counter)");
  if (count == 0) return GS_OK;
  if (!out) return fail(c, GS_ERR_ARG, "null pointer");
  if (!host) return rand_fr_launch(c, domain, stream, first, count, out);
  return staged_call(c, {}, {{out, count * SZ_FR}},
                     [&](void** d) { return rand_fr_launch(c, domain, stream, first, count, d[0]); });
}
int gs_rand_fr_dev(gs_ctx* c, uint32_t domain, uint64_t stream, uint64_t first, size_t count, void* out) {
  return rand_fr_call(c, "gs_rand_fr_dev", false, domain, stream, first, count, out);
}
int gs_rand_fr(gs_ctx* c, uint32_t domain, uint64_t stream, uint64_t first, size_t count, void* out) {
  return rand_fr_call(c, "gs_rand_fr", true, domain, stream, first, count, out);
}
static int rand_rho_call(gs_ctx* c, const char* fn, bool host, uint64_t stream, uint64_t first, size_t count,
                         uint64_t* out) {
  RC(rand_check(c, fn));
  // blocks first div 8 .. (first + count - 1) div 8, all below 2^32 (first + count itself must not wrap either)
  if (first > 8 * RAND_COUNTERS || (uint64_t)count > 8 * RAND_COUNTERS - first)
    return fail(c, GS_ERR_SHAPE, "gs_rand_rho: (first + count + 7) div 8 > 2^32 (eight exponents per block, 32-bit block counter)");
  if (count == 0) return GS_OK;
  if (!out) return fail(c, GS_ERR_ARG, "null pointer");
  const size_t nblocks = (size_t)((first + count + 7) / 8 - first / 8);
  auto go = [&](uint64_t* d) {
    return launch(c, "k_rand_rho", k_rand_rho, nblocks, RAND_BLOCK, nblocks, (const uint32_t*)c->rkey.p, stream, first,
                  (uint64_t)count, d);
  };
  if (!host) return go(out);
  return staged_call(c, {}, {{out, count * sizeof(uint64_t)}}, [&](void** d) { return go((uint64_t*)d[0]); });
}
int gs_rand_rho_dev(gs_ctx* c, uint64_t stream, uint64_t first, size_t count, uint64_t* out) {
  return rand_rho_call(c, "gs_rand_rho_dev", false, stream, first, count, out);
}
int gs_rand_rho(gs_ctx* c, uint64_t stream, uint64_t first, size_t count, uint64_t* out) {
  return rand_rho_call(c, "gs_rand_rho", true, stream, first, count, out);
}

// The drawn forms of prove and rerandomize: the sibling's arrays with R, S, T as optional OUTPUTS, and a run that draws
// the three arrays (asked for: into the caller's / the pipe's buffer; else into scratch that is zeroed behind the
// sibling's kernels) and then runs the sibling.  sr = the slot of R (S and T follow it), dom = the domain of R.
static_assert(PI_S == PI_R + 1 && PI_T == PI_R + 2 && RI_S == RI_R + 1 && RI_T == RI_R + 2, "R, S, T are consecutive slots");
static_assert(GS_RAND_PROVE_S == GS_RAND_PROVE_R + 1 && GS_RAND_PROVE_T == GS_RAND_PROVE_R + 2 &&
                  GS_RAND_RERAND_S == GS_RAND_RERAND_R + 1 && GS_RAND_RERAND_T == GS_RAND_RERAND_R + 2,
              "the domains of R, S, T are consecutive");
static int drawn_run(gs_ctx* c, const BatchArgs& a, const Op& sibling, int sr, uint32_t dom) {
  static const char* const names[3] = {"drawn.R", "drawn.S", "drawn.T"};
  static const lay::Array arrs[3] = {lay::R, lay::S, lay::T};
  const lay::Layout L = layout_of(c, a);
  struct Wipe {  // whatever happens below: on the stream, after the kernels enqueued so far
    gs_ctx* c;
    void* p[3];
    size_t bytes[3];
    ~Wipe() {
      for (int k = 0; k < 3; k++)
        if (p[k]) hipMemsetAsync(p[k], 0, bytes[k], c->stream);
    }
  } wipe{c, {nullptr, nullptr, nullptr}, {0, 0, 0}};
  BatchArgs d = a;
  for (int k = 0; k < 3; k++) {
    const size_t bytes = L.bytes[arrs[k]];
    void* p = a.out(sr + k);
    if (!p) {
      RC(scratch(c, names[k], bytes, &p));
      wipe.p[k] = p, wipe.bytes[k] = bytes;
      d.p[sr + k] = p;
    }
    RC(rand_fr_launch(c, dom + k, a.stream, 0, bytes / SZ_FR, p));
  }
  return sibling.run(c, d);
}
static const ArrDesc kProveDrawnArrs[] = {
    {PI_X, lay::X, ARR_IN},      {PI_Y, lay::Y, ARR_IN},      {PI_A, lay::A, ARR_IN},
    {PI_B, lay::B, ARR_IN},      {PI_G, lay::GAMMA, ARR_IN},  {PI_R, lay::R, ARR_OUT | ARR_OPT},
    {PI_S, lay::S, ARR_OUT | ARR_OPT}, {PI_T, lay::T, ARR_OUT | ARR_OPT}, {PO_XC, lay::XCOMS, ARR_OUT | ARR_OPT},
    {PO_YC, lay::YCOMS, ARR_OUT | ARR_OPT}, {PO_PI, lay::PI, ARR_OUT}, {PO_TH, lay::THETA, ARR_OUT}};
static const int* prove_drawn_order(int) {
  static const int order[] = {PI_G, PI_Y, PI_B, PI_X, PI_A};  // prove_order without the scalars that are drawn
  return order;
}
static int prove_drawn_run(gs_ctx* c, const BatchArgs& a) { return drawn_run(c, a, kProve, PI_R, GS_RAND_PROVE_R); }
static const Op kProveDrawn = {kProveDrawnArrs, sizeof kProveDrawnArrs / sizeof *kProveDrawnArrs, prove_drawn_order, 5,
                               prove_drawn_run};
static const ArrDesc kRerandDrawnArrs[] = {
    {RI_A, lay::A, ARR_IN},       {RI_B, lay::B, ARR_IN},       {RI_G, lay::GAMMA, ARR_IN},
    {RI_R, lay::R, ARR_OUT | ARR_OPT}, {RI_S, lay::S, ARR_OUT | ARR_OPT}, {RI_T, lay::T, ARR_OUT | ARR_OPT},
    {RI_XC, lay::XCOMS, ARR_IN},  {RI_YC, lay::YCOMS, ARR_IN},  {RI_PI, lay::PI, ARR_IN},   {RI_TH, lay::THETA, ARR_IN},
    {RO_XC, lay::XCOMS, ARR_OUT}, {RO_YC, lay::YCOMS, ARR_OUT}, {RO_PI, lay::PI, ARR_OUT},  {RO_TH, lay::THETA, ARR_OUT}};
static const int* rerand_drawn_order(int) {
  static const int order[] = {RI_G, RI_B, RI_A, RI_YC, RI_PI, RI_XC, RI_TH};  // rerand_order without the scalars
  return order;
}
static int rerand_drawn_run(gs_ctx* c, const BatchArgs& a) { return drawn_run(c, a, kRerand, RI_R, GS_RAND_RERAND_R); }
static const Op kRerandDrawn = {kRerandDrawnArrs, sizeof kRerandDrawnArrs / sizeof *kRerandDrawnArrs, rerand_drawn_order, 7,
                                rerand_drawn_run};
static int drawn_call(gs_ctx* c, const char* fn, const Op& op, bool host, const BatchArgs& a) {
  if (c && c->rec) return fail(c, GS_ERR_ARG, (std::string(fn) + " inside a mixed call").c_str());
  RC(batch_check(c, op, a));
  if (!c->have_rkey) return fail(c, GS_ERR_ARG, (std::string(fn) + ": gs_rand_set_key has not been called").c_str());
  if (a.N == 0) return GS_OK;
  const lay::Layout L = layout_of(c, a);
  for (lay::Array r : {lay::R, lay::S, lay::T})
    if (L.bytes[r] / SZ_FR > RAND_COUNTERS)
      return fail(c, GS_ERR_SHAPE, (std::string(fn) + ": more than 2^32 scalars in one of R, S, T").c_str());
  if (!host) return op.run(c, a);
  // outputs do not alias inputs or each other (the staged copies would hide it; the device form's contract)
  for (int oi = 0; oi < op.narrs; oi++) {
    const ArrDesc& o = op.arrs[oi];
    if (!(o.flags & ARR_OUT) || !a.p[o.slot]) continue;
    for (int ii = 0; ii < op.narrs; ii++) {
      const ArrDesc& i = op.arrs[ii];
      if (i.slot == o.slot || !a.p[i.slot]) continue;
      uintptr_t x = (uintptr_t)a.p[o.slot], y = (uintptr_t)a.p[i.slot];
      if (x < y + L.bytes[i.arr] && y < x + L.bytes[o.arr])
        return fail(c, GS_ERR_ARG, (std::string(fn) + ": an output overlaps another array").c_str());
    }
  }
  return batch_host_checked(c, op, a);
}
static BatchArgs with_stream(BatchArgs a, uint64_t stream) {
  a.stream = stream;
  return a;
}
#define GS_PROVE_DRAWN_ENTRY(NAME, HOST, SHARED)                                                                      \
  int NAME(gs_ctx* c, int ty, size_t N, int m, int n, const void* X, const void* Y, const void* A, const void* B,      \
           const void* G, uint64_t stream, void* R, void* S, void* T, void* xcoms, void* ycoms, void* pi, void* theta) { \
    return drawn_call(c, #NAME, kProveDrawn, HOST,                                                                     \
                      with_stream(BatchArgs{ty, N, m, n, SHARED, {X, Y, A, B, G, R, S, T, xcoms, ycoms, pi, theta}}, stream)); \
  }
GS_PROVE_DRAWN_ENTRY(gs_prove_batch_drawn_dev, false, false)
GS_PROVE_DRAWN_ENTRY(gs_prove_batch_drawn, true, false)
GS_PROVE_DRAWN_ENTRY(gs_prove_statement_drawn_dev, false, true)
GS_PROVE_DRAWN_ENTRY(gs_prove_statement_drawn, true, true)
#undef GS_PROVE_DRAWN_ENTRY
#define GS_RERAND_DRAWN_ENTRY(NAME, HOST, SHARED)                                                                     \
  int NAME(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G, const void* xcoms,  \
           const void* ycoms, const void* pi, const void* theta, uint64_t stream, void* R, void* S, void* T,          \
           void* xcoms_out, void* ycoms_out, void* pi_out, void* theta_out) {                                         \
    return drawn_call(c, #NAME, kRerandDrawn, HOST,                                                                    \
                      with_stream(rerand_args(ty, N, m, n, SHARED, A, B, G, xcoms, ycoms, pi, theta, R, S, T, xcoms_out, \
                                              ycoms_out, pi_out, theta_out),                                          \
                                  stream));                                                                            \
  }
GS_RERAND_DRAWN_ENTRY(gs_rerandomize_batch_drawn_dev, false, false)
GS_RERAND_DRAWN_ENTRY(gs_rerandomize_batch_drawn, true, false)
GS_RERAND_DRAWN_ENTRY(gs_rerandomize_statement_drawn_dev, false, true)
GS_RERAND_DRAWN_ENTRY(gs_rerandomize_statement_drawn, true, true)
#undef GS_RERAND_DRAWN_ENTRY

// ---- witness extraction with the binding key ---------------------------------------
int gs_set_extraction_key(gs_ctx* c, const void* a1a2) {
  RC(check_ctx(c, false));
  clear_extraction_key(c);
  if (!a1a2) return GS_OK;
  RC(check_ctx(c, true));
  if (c->rec) return fail(c, GS_ERR_ARG, "gs_set_extraction_key inside a mixed call");
  int rc = DISPATCH_FN(c, set_extraction_key_impl, (c, a1a2));
  if (rc != GS_OK) clear_extraction_key(c);  // a refused key leaves nothing behind
  return rc;
}

static int extract_check(gs_ctx* c, size_t n, const void* coms, void* out, size_t pt) {
  RC(check_ctx(c, true));
  if (!c->have_xkey) return fail(c, GS_ERR_ARG, "gs_set_extraction_key has not been called");
  if (n == 0) return GS_OK;
  if (!coms || !out) return fail(c, GS_ERR_ARG, "null pointer");
  const uint8_t *a = (const uint8_t*)coms, *b = (const uint8_t*)out;
  if (a < b + n * pt && b < a + 2 * n * pt) return fail(c, GS_ERR_ARG, "gs_extract: out overlaps coms");
  return GS_OK;
}
int gs_extract_g1_dev(gs_ctx* c, size_t n, const void* coms, void* out) {
  RC(extract_check(c, n, coms, out, c ? 2 * sz_fq(c->curve) : 0));
  if (n == 0) return GS_OK;
  return WIRE_DISPATCH((extract_impl<Bls12_381, Fq<Bls12_381>>(c, "k_extract.g1", 0, n, coms, out)),
                       (extract_impl<Bn254, Fq<Bn254>>(c, "k_extract.g1", 0, n, coms, out)));
}
int gs_extract_g2_dev(gs_ctx* c, size_t n, const void* coms, void* out) {
  RC(extract_check(c, n, coms, out, c ? 4 * sz_fq(c->curve) : 0));
  if (n == 0) return GS_OK;
  return WIRE_DISPATCH((extract_impl<Bls12_381, Fp2<Bls12_381>>(c, "k_extract.g2", 2, n, coms, out)),
                       (extract_impl<Bn254, Fp2<Bn254>>(c, "k_extract.g2", 2, n, coms, out)));
}
static int extract_host(gs_ctx* c, bool g2, size_t n, const void* coms, void* out) {
  RC(check_ctx(c, true));
  if (!c->have_xkey) return fail(c, GS_ERR_ARG, "gs_set_extraction_key has not been called");
  if (n == 0) return GS_OK;
  if (!coms || !out) return fail(c, GS_ERR_ARG, "null pointer");
  const size_t pt = (g2 ? 4 : 2) * sz_fq(c->curve);
  return staged_call(c, {{coms, n * 2 * pt}}, {{out, n * pt}},
                     [&](void** d) { return (g2 ? gs_extract_g2_dev : gs_extract_g1_dev)(c, n, d[0], d[1]); });
}
int gs_extract_g1(gs_ctx* c, size_t n, const void* coms, void* out) { return extract_host(c, false, n, coms, out); }
int gs_extract_g2(gs_ctx* c, size_t n, const void* coms, void* out) { return extract_host(c, true, n, coms, out); }

// ---- bounded discrete logarithms: baby-step giant-step (csrc/gs_kernels.cuh: k_dlog_table, k_dlog) ------------------
}  // extern "C"
static const size_t DLOG_AUX_STEPS = 256;  // offset of the giant steps behind the base point in DlogTab::aux
template <class C, class F> static int dlog_prepare_impl(gs_ctx* c, int gi, const void* base_host, unsigned log2_table) {
  gs_ctx::DlogTab& t = c->dlog[gi];
  const size_t pt = AFFB(C, F);
  static_assert(AFFB(C, F) <= DLOG_AUX_STEPS, "base point in front of the giant steps");
  constexpr int K = DlogShape<F>::K;
  const size_t slot_bytes = sizeof(uint64_t) << (log2_table + 1);
  // replace: nothing enqueued may still read the old table; the old one is freed before the new one is asked for
  HIPCHK(c, hipStreamSynchronize(c->stream));
  t.ready = false;
  if (t.slots.p && t.slots.cap != slot_bytes) {
    hipFree(t.slots.p);
    t.slots = DevBuf();
  }
  if (!t.slots.p) {
    hipError_t e = hipMalloc(&t.slots.p, slot_bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      t.slots = DevBuf();
      return fail(c, GS_ERR_ALLOC, "gs_dlog_prepare: the table does not fit (2^(log2_table+1) slots of 8 bytes)", e);
    }
    t.slots.cap = slot_bytes;
  }
  RC(ensure(c, t.aux, DLOG_AUX_STEPS + K * sizeof(Aff<F>)));
  uint8_t* aux = (uint8_t*)t.aux.p;
  HIPCHK(c, hipMemcpyAsync(aux, base_host, pt, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(t.slots.p, 0, slot_bytes, c->stream));
  const size_t B = (size_t)1 << log2_table;
  const int run = B < (size_t)DLOG_RUN ? (int)B : DLOG_RUN;
  const char* names[2][2] = {{"k_dlog_table.g1", "k_dlog_steps.g1"}, {"k_dlog_table.g2", "k_dlog_steps.g2"}};
  c->work_hint = B;
  RC(launch_seg<k_dlog_table<C, F>>(c, names[gi][0], B / run, 64, B / run, (const uint8_t*)aux, run, log2_table + 1,
                                    (unsigned long long*)t.slots.p));
  RC(launch(c, names[gi][1], k_dlog_steps<C, F>, K, 64, (const uint8_t*)aux, (uint64_t)(2 * B), K,
            (Aff<F>*)(aux + DLOG_AUX_STEPS)));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // base_host is the caller's again
  t.log2_table = log2_table;
  t.ready = true;
  return GS_OK;
}
// pts, out, found: device pointers; checked by the caller
template <class C, class F>
static int dlog_run_impl(gs_ctx* c, int gi, size_t n, const void* pts, unsigned bits, void* out, void* found) {
  const gs_ctx::DlogTab& t = c->dlog[gi];
  const uint8_t* aux = (const uint8_t*)t.aux.p;
  const unsigned T = t.log2_table;
  const uint64_t centres = bits > T + 1 ? (uint64_t)1 << (bits - T - 1) : 1;  // stride 2^(T+1) over [0, 2^bits)
  const uint64_t per = c->dlog_steps ? (uint64_t)c->dlog_steps : (uint64_t)DLOG_STEPS_DEFAULT;
  const unsigned fpb = c->dlog_fp_bits ? (unsigned)c->dlog_fp_bits : (unsigned)DLOG_FP_BITS;
  const char* name = gi == 0 ? "k_dlog.g1" : "k_dlog.g2";
  for (uint64_t t0 = 0; t0 < centres; t0 += per) {
    const uint32_t ns = (uint32_t)std::min(per, centres - t0);
    c->work_hint = (uint64_t)n * ns;
    RC(launch_seg<k_dlog<C, F>>(c, name, n, 64, n, (const uint8_t*)pts, aux, (const Aff<F>*)(aux + DLOG_AUX_STEPS),
                                (const unsigned long long*)t.slots.p, T + 1, T, bits, fpb, t0, ns, t0 == 0 ? 1 : 0,
                                (Fr<C>*)out, (uint8_t*)found));
  }
  return GS_OK;
}
static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uint8_t *x = (const uint8_t*)a, *y = (const uint8_t*)b;
  return x < y + nb && y < x + na;
}
// everything gs_dlog_* refuses, in one place; in_bytes = bytes of the input array per element
static int dlog_check(gs_ctx* c, const char* fn, int gi, size_t n, const void* in, size_t in_bytes, unsigned bits,
                      void* out, void* found) {
  if (c->rec) return fail(c, GS_ERR_ARG, (std::string(fn) + " inside a mixed call").c_str());
  const gs_ctx::DlogTab& t = c->dlog[gi];
  if (!t.ready) return fail(c, GS_ERR_ARG, (std::string(fn) + ": gs_dlog_prepare has not been called for this group").c_str());
  if (bits < 1 || bits > 48) return fail(c, GS_ERR_ARG, (std::string(fn) + ": bits must be 1 .. 48").c_str());
  if (bits > t.log2_table + 25) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: bits = %u needs more than 2^24 giant steps with log2_table = %u; prepare log2_table >= %u",
             fn, bits, t.log2_table, bits - 25);
    return fail(c, GS_ERR_ARG, msg);
  }
  if (n == 0) return GS_OK;
  if (!in || !out || !found) return fail(c, GS_ERR_ARG, "null pointer");
  if (ranges_overlap(in, n * in_bytes, out, n * SZ_FR) || ranges_overlap(in, n * in_bytes, found, n) ||
      ranges_overlap(out, n * SZ_FR, found, n))
    return fail(c, GS_ERR_ARG, (std::string(fn) + ": outputs overlap the input or each other").c_str());
  return GS_OK;
}
static int dlog_dev(gs_ctx* c, const char* fn, int gi, size_t n, const void* pts, unsigned bits, void* out, void* found) {
  RC(check_ctx(c, false));
  RC(dlog_check(c, fn, gi, n, pts, (gi ? 4 : 2) * sz_fq(c->curve), bits, out, found));
  if (n == 0) return GS_OK;
  if (gi == 0)
    return WIRE_DISPATCH((dlog_run_impl<Bls12_381, Fq<Bls12_381>>(c, 0, n, pts, bits, out, found)),
                         (dlog_run_impl<Bn254, Fq<Bn254>>(c, 0, n, pts, bits, out, found)));
  return WIRE_DISPATCH((dlog_run_impl<Bls12_381, Fp2<Bls12_381>>(c, 1, n, pts, bits, out, found)),
                       (dlog_run_impl<Bn254, Fp2<Bn254>>(c, 1, n, pts, bits, out, found)));
}
// k_extract into context scratch, then the walk over the images
static int extract_scalar_dev(gs_ctx* c, const char* fn, int gi, size_t n, const void* coms, unsigned bits, void* out,
                              void* found) {
  RC(check_ctx(c, true));
  if (!c->have_xkey) return fail(c, GS_ERR_ARG, "gs_set_extraction_key has not been called");
  const size_t pt = (gi ? 4 : 2) * sz_fq(c->curve);
  RC(dlog_check(c, fn, gi, n, coms, 2 * pt, bits, out, found));
  if (n == 0) return GS_OK;
  void* img;
  RC(scratch(c, gi ? "xs.img2" : "xs.img1", n * pt, &img));
  RC(gi ? gs_extract_g2_dev(c, n, coms, img) : gs_extract_g1_dev(c, n, coms, img));
  return dlog_dev(c, fn, gi, n, img, bits, out, found);
}
// the host forms: stage in, run the _dev form, copy both outputs back
static int dlog_host(gs_ctx* c, const char* fn, int gi, bool coms, size_t n, const void* in, unsigned bits, void* out,
                     void* found) {
  RC(check_ctx(c, coms));
  if (coms && !c->have_xkey) return fail(c, GS_ERR_ARG, "gs_set_extraction_key has not been called");
  const size_t in_bytes = (coms ? 2 : 1) * (gi ? 4 : 2) * sz_fq(c->curve);
  RC(dlog_check(c, fn, gi, n, in, in_bytes, bits, out, found));
  if (n == 0) return GS_OK;
  return staged_call(c, {{in, n * in_bytes}}, {{out, n * SZ_FR}, {found, n}}, [&](void** d) {
    return (coms ? extract_scalar_dev : dlog_dev)(c, fn, gi, n, d[0], bits, d[1], d[2]);
  });
}
// k P for n points of G1 (FT = Fq) or G2 (FT = Fp2), `grp` = ".g1" / ".g2"
template <template <class> class FT>
static int mul_batch_dev(gs_ctx* c, const char* grp, size_t n, const void* p, int bc, const void* k, void* out) {
  RC(check_ctx(c, false));
  if (n == 0) return GS_OK;
  typedef Bls12_381 C0;
  typedef Bn254 C1;
  const std::string name = std::string(c->endo ? "k_smul_batch" : "k_smul_batch.plain") + grp;
  auto go = [&](auto kern, auto* s) { return launch(c, name.c_str(), kern, n, 64, n, (const uint8_t*)p, bc, s, (uint8_t*)out); };
  if (!c->endo)  // plain double-and-add lanes: any curve point (gs_set_option "endo" 0)
    return c->curve == 0 ? go(k_smul_batch<C0, FT<C0>, false>, (const Fr<C0>*)k)
                         : go(k_smul_batch<C1, FT<C1>, false>, (const Fr<C1>*)k);
  return c->curve == 0 ? go(k_smul_batch<C0, FT<C0>>, (const Fr<C0>*)k) : go(k_smul_batch<C1, FT<C1>>, (const Fr<C1>*)k);
}
extern "C" {
int gs_dlog_prepare(gs_ctx* c, int group, const void* base_host, unsigned log2_table) {
  RC(check_ctx(c, false));
  if (c->rec) return fail(c, GS_ERR_ARG, "gs_dlog_prepare inside a mixed call");
  if (group != 1 && group != 2) return fail(c, GS_ERR_ARG, "gs_dlog_prepare: group must be 1 or 2");
  if (log2_table < 2 || log2_table > 28) return fail(c, GS_ERR_ARG, "gs_dlog_prepare: log2_table must be 2 .. 28");
  if (!base_host) return fail(c, GS_ERR_ARG, "null pointer");
  const size_t pt = (group == 2 ? 4 : 2) * sz_fq(c->curve);
  bool zero = true;
  for (size_t i = 0; i < pt; i++) zero = zero && ((const uint8_t*)base_host)[i] == 0;
  if (zero) return fail(c, GS_ERR_ARG, "gs_dlog_prepare: the base is the identity");
  if (group == 1)
    return WIRE_DISPATCH((dlog_prepare_impl<Bls12_381, Fq<Bls12_381>>(c, 0, base_host, log2_table)),
                         (dlog_prepare_impl<Bn254, Fq<Bn254>>(c, 0, base_host, log2_table)));
  return WIRE_DISPATCH((dlog_prepare_impl<Bls12_381, Fp2<Bls12_381>>(c, 1, base_host, log2_table)),
                       (dlog_prepare_impl<Bn254, Fp2<Bn254>>(c, 1, base_host, log2_table)));
}
int gs_dlog_g1_dev(gs_ctx* c, size_t n, const void* pts, unsigned bits, void* out, void* found) {
  return dlog_dev(c, "gs_dlog_g1_dev", 0, n, pts, bits, out, found);
}
int gs_dlog_g2_dev(gs_ctx* c, size_t n, const void* pts, unsigned bits, void* out, void* found) {
  return dlog_dev(c, "gs_dlog_g2_dev", 1, n, pts, bits, out, found);
}
int gs_dlog_g1(gs_ctx* c, size_t n, const void* pts, unsigned bits, void* out, void* found) {
  return dlog_host(c, "gs_dlog_g1", 0, false, n, pts, bits, out, found);
}
int gs_dlog_g2(gs_ctx* c, size_t n, const void* pts, unsigned bits, void* out, void* found) {
  return dlog_host(c, "gs_dlog_g2", 1, false, n, pts, bits, out, found);
}
int gs_extract_scalar_b1_dev(gs_ctx* c, size_t n, const void* coms, unsigned bits, void* out, void* found) {
  return extract_scalar_dev(c, "gs_extract_scalar_b1_dev", 0, n, coms, bits, out, found);
}
int gs_extract_scalar_b2_dev(gs_ctx* c, size_t n, const void* coms, unsigned bits, void* out, void* found) {
  return extract_scalar_dev(c, "gs_extract_scalar_b2_dev", 1, n, coms, bits, out, found);
}
int gs_extract_scalar_b1(gs_ctx* c, size_t n, const void* coms, unsigned bits, void* out, void* found) {
  return dlog_host(c, "gs_extract_scalar_b1", 0, true, n, coms, bits, out, found);
}
int gs_extract_scalar_b2(gs_ctx* c, size_t n, const void* coms, unsigned bits, void* out, void* found) {
  return dlog_host(c, "gs_extract_scalar_b2", 1, true, n, coms, bits, out, found);
}

// ---- helpers / hooks -----------------------------------------------------------
int gs_g1_mul_batch_dev(gs_ctx* c, size_t n, const void* p, int bc, const void* k, void* out) {
  return mul_batch_dev<Fq>(c, ".g1", n, p, bc, k, out);
}
int gs_g2_mul_batch_dev(gs_ctx* c, size_t n, const void* p, int bc, const void* k, void* out) {
  return mul_batch_dev<Fp2>(c, ".g2", n, p, bc, k, out);
}
static int mul_batch_host(gs_ctx* c, bool g2, size_t n, const void* p, int bc, const void* k, void* out) {
  RC(check_ctx(c, false));
  const size_t pt = (g2 ? 4 : 2) * sz_fq(c->curve);  // boundary bytes of one point
  return staged_call(c, {{p, (bc ? 1 : n) * pt}, {k, n * SZ_FR}}, {{out, n * pt}}, [&](void** d) {
    return (g2 ? gs_g2_mul_batch_dev : gs_g1_mul_batch_dev)(c, n, d[0], bc, d[1], d[2]);
  });
}
int gs_g1_mul_batch(gs_ctx* c, size_t n, const void* p, int bc, const void* k, void* out) {
  return mul_batch_host(c, false, n, p, bc, k, out);
}
int gs_g2_mul_batch(gs_ctx* c, size_t n, const void* p, int bc, const void* k, void* out) {
  return mul_batch_host(c, true, n, p, bc, k, out);
}

int gs_multi_pairing_batch_dev(gs_ctx* c, size_t n, int k, const void* p, const void* q, void* out) {
  RC(check_ctx(c, false));
  if (n == 0) return GS_OK;
  if (k < 0) return GS_ERR_ARG;
  if (c->curve == 0)
    return launch(c, "k_multi_pairing", k_multi_pairing<Bls12_381>, n, 64, n, k, (const uint8_t*)p,
                  (const uint8_t*)q, (uint8_t*)out);
  return launch(c, "k_multi_pairing", k_multi_pairing<Bn254>, n, 64, n, k, (const uint8_t*)p, (const uint8_t*)q,
                (uint8_t*)out);
}
int gs_multi_pairing_batch(gs_ctx* c, size_t n, int k, const void* p, const void* q, void* out) {
  RC(check_ctx(c, false));
  const size_t fq = sz_fq(c->curve);
  return staged_call(c, {{p, n * k * 2 * fq}, {q, n * k * 4 * fq}}, {{out, n * 12 * fq}},
                     [&](void** d) { return gs_multi_pairing_batch_dev(c, n, k, d[0], d[1], d[2]); });
}

int gs_gt_pow_batch_dev(gs_ctx* c, size_t n, const void* base, const void* k, void* out) {
  RC(check_ctx(c, false));
  if (n == 0) return GS_OK;
  if (c->curve == 0)
    return launch(c, "k_gt_pow", k_gt_pow<Bls12_381>, n, 64, n, (const uint8_t*)base, (const Fr<Bls12_381>*)k,
                  (uint8_t*)out);
  return launch(c, "k_gt_pow", k_gt_pow<Bn254>, n, 64, n, (const uint8_t*)base, (const Fr<Bn254>*)k, (uint8_t*)out);
}

// ComT::pairing_sum: four multi-pairings over the component selections (a,b)
int gs_pairing_sum(gs_ctx* c, int k, const void* x, const void* y, void* out) {
  RC(check_ctx(c, false));
  if (k < 0) return GS_ERR_ARG;
  size_t fq = sz_fq(c->curve);
  size_t g1 = 2 * fq, g2 = 4 * fq;
  std::vector<uint8_t> P(4 * (size_t)k * g1 + 1), Q(4 * (size_t)k * g2 + 1);
  const uint8_t* xb = (const uint8_t*)x;
  const uint8_t* yb = (const uint8_t*)y;
  for (int cell = 0; cell < 4; cell++) {
    int a = cell >> 1, b = cell & 1;
    for (int i = 0; i < k; i++) {
      memcpy(&P[((size_t)cell * k + i) * g1], xb + (size_t)i * 2 * g1 + a * g1, g1);
      memcpy(&Q[((size_t)cell * k + i) * g2], yb + (size_t)i * 2 * g2 + b * g2, g2);
    }
  }
  return gs_multi_pairing_batch(c, 4, k, P.data(), Q.data(), out);
}

int gs_mat_left_mul_com1(gs_ctx* c, int rows, int k, const void* lhs, const void* col, void* out) {
  RC(check_ctx(c, false));
  if (rows <= 0 || k <= 0) return GS_OK;  // empty product (data_structures.rs:697-702)
  return WIRE_DISPATCH((left_mul_impl<Bls12_381, Fq<Bls12_381>>(c, rows, k, lhs, col, out)),
                       (left_mul_impl<Bn254, Fq<Bn254>>(c, rows, k, lhs, col, out)));
}
int gs_mat_left_mul_com2(gs_ctx* c, int rows, int k, const void* lhs, const void* col, void* out) {
  RC(check_ctx(c, false));
  if (rows <= 0 || k <= 0) return GS_OK;
  return WIRE_DISPATCH((left_mul_impl<Bls12_381, Fp2<Bls12_381>>(c, rows, k, lhs, col, out)),
                       (left_mul_impl<Bn254, Fp2<Bn254>>(c, rows, k, lhs, col, out)));
}

int gs_fr_matmul(gs_ctx* c, int rows, int inner, int cols, const void* lhs, const void* rhs, void* out) {
  RC(check_ctx(c, false));
  if (rows <= 0 || inner <= 0 || cols <= 0) return GS_OK;  // empty product
  if (!lhs || !rhs || !out) return fail(c, GS_ERR_ARG, "null pointer");
  if (rows > 4096 || inner > 4096 || cols > 4096) return fail(c, GS_ERR_SHAPE, "matrix too large");
  return WIRE_DISPATCH(fr_matmul_impl<Bls12_381>(c, rows, inner, cols, lhs, rhs, out),
                       fr_matmul_impl<Bn254>(c, rows, inner, cols, lhs, rhs, out));
}

// ---- batched (RLC) verifiers: one combined check per batch, the same with fault localisation, one per Statement, one
// per batch of proofs of ONE equation -----
// All four move the verifier's eight inputs, the exponents rho and up to three outputs.  rlc_arrays states a call's
// arrays ONCE; the checks of the eight entry points and the staging of the four host forms walk that list.
enum RlcVariant { RLC_PLAIN, RLC_LOCATE, RLC_STMT, RLC_EQ };
enum { RLC_RHO = 8, RLC_ACC, RLC_OK, RLC_INFO, RLC_MAX };
struct RlcCall {
  RlcVariant v;
  int ty;
  size_t S, N;  // RLC_STMT: S statements of N = E equations each over shared commitments; otherwise S = 1
                // (RLC_EQ: N proofs of one equation -- A, B, Gamma, target are ONE copy)
  int m, n;
  // A, B, Gamma, target, xcoms, ycoms, pi, theta, rho, acc, ok (not RLC_PLAIN), info (RLC_LOCATE): host pointers at the
  // un-suffixed entry points, device pointers at the _dev ones and inside
  const void* p[RLC_MAX];
  void* out(int i) const { return const_cast<void*>(p[i]); }
};
struct RlcArr {
  const char* name;
  const void* p;
  size_t bytes;
  int flags;  // ARR_IN / ARR_OUT; ARR_OPT: may be NULL in the host form (a _dev form requires every array)
};
// a[i] describes k.p[i]; returns how many the variant has
static int rlc_arrays(const gs_ctx* c, const RlcCall& k, RlcArr* a) {
  static const lay::Array in[8] = {lay::A, lay::B, lay::GAMMA, lay::TARGET, lay::XCOMS, lay::YCOMS, lay::PI, lay::THETA};
  const size_t fq = sz_fq(c->curve);
  // one statement = the shared layout with N = E; RLC_EQ: the layout whose constants are one copy
  const lay::Layout L = k.v == RLC_EQ ? lay::Layout::one_equation(fq, k.ty, k.N, k.m, k.n)
                                      : lay::Layout(fq, k.ty, k.N, k.m, k.n, k.v == RLC_STMT);
  int na = 0;
  for (; na < 8; na++) a[na] = {lay::kArrayName[in[na]], k.p[na], k.S * L.bytes[in[na]], ARR_IN};
  a[na++] = {"rho", k.p[RLC_RHO], 4 * k.S * k.N * sizeof(uint64_t), ARR_IN};        // four exponents per equation
  a[na++] = {"acc", k.p[RLC_ACC], k.S * 2 * 12 * fq, ARR_OUT | ARR_OPT};            // one GT pair per combined check
  if (k.v == RLC_LOCATE || k.v == RLC_STMT) a[na++] = {"ok", k.p[RLC_OK], k.v == RLC_STMT ? k.S : k.N, ARR_OUT};
  if (k.v == RLC_LOCATE) a[na++] = {"info", k.p[RLC_INFO], 2 * sizeof(uint32_t), ARR_OUT | ARR_OPT};
  return na;
}
// everything the eight entry points refuse; fills a[] / *na for the caller
static int rlc_check(gs_ctx* c, const RlcCall& k, bool host, RlcArr* a, int* na) {
  RC(check_ctx(c, true));
  if (k.v == RLC_EQ && c->rec) return fail(c, GS_ERR_ARG, "gs_verify_equation_rlc inside a mixed call");
  RC(check_shape(c, k.ty, k.m, k.n));
  if (k.S == 0 || k.N == 0)
    return fail(c, GS_ERR_ARG, k.v == RLC_STMT ? "empty batch: S and E must be >= 1" : "empty batch");
  // what the plan cannot index is refused
  if (k.v == RLC_LOCATE && k.N >= ((size_t)1 << 32) / 8)
    return fail(c, GS_ERR_SHAPE, "gs_verify_batch_rlc_locate: node indices are 32-bit");
  if (k.v == RLC_EQ && k.N >= ((size_t)1 << 32))  // the halves of rho are summed in 64 bits (k_prep_verify_eq_rlc)
    return fail(c, GS_ERR_SHAPE, "gs_verify_equation_rlc: at most 2^32 - 1 proofs per call");
  if (k.v == RLC_STMT) {  // arrays strided per STATEMENT in 32-bit bytes, 32-bit task tables and pool offsets
    const size_t E = k.N, lim = (size_t)1 << 32;
    const int m = k.m, n = k.n;
    const lay::Layout L(sz_fq(c->curve), k.ty, E, m, n, true);
    if (E > ((size_t)1 << 20) || L.bytes[lay::A] >= lim || L.bytes[lay::B] >= lim || L.bytes[lay::TARGET] >= lim ||
        L.bytes[lay::PI] >= lim || L.bytes[lay::THETA] >= lim || L.bytes[lay::XCOMS] >= lim ||
        L.bytes[lay::YCOMS] >= lim || E * (size_t)(4 + 4 * (m + n)) + 4 * (size_t)m * n * 4 >= ((size_t)1 << 28))
      return fail(c, GS_ERR_SHAPE, "statement too large for the task tables (E x shape)");
  }
  *na = rlc_arrays(c, k, a);
  for (int i = 0; i < *na; i++)
    if (!a[i].p && !(host && (a[i].flags & ARR_OPT)))
      return fail(c, GS_ERR_ARG, (std::string("null pointer: ") + a[i].name).c_str());
  if (!host) return GS_OK;  // device pointers: nothing to read, and whether they overlap is the caller's business
  const uint64_t* rho = (const uint64_t*)k.p[RLC_RHO];
  for (size_t i = 0; i < 4 * k.S * k.N; i++)  // a zero exponent drops its cell equation from every check it is part of
    if (rho[i] == 0) return fail(c, GS_ERR_ARG, "rho must be non-zero (see the rho contract in gs_amd.h)");
  if (k.v != RLC_LOCATE) return GS_OK;
  for (int o = 0; o < *na; o++) {  // no output may lie over an input or over another output
    if (!(a[o].flags & ARR_OUT) || !a[o].p) continue;
    for (int i = 0; i < o; i++)
      if (a[i].p && ranges_overlap(a[o].p, a[o].bytes, a[i].p, a[i].bytes))
        return fail(c, GS_ERR_ARG, a[i].flags & ARR_OUT ? "gs_verify_batch_rlc_locate: the outputs overlap each other"
                                                        : "gs_verify_batch_rlc_locate: an output overlaps an input");
  }
  return GS_OK;
}
// the kernels of a checked call (device pointers)
static int rlc_run(gs_ctx* c, const RlcCall& k) {
  const VerifyIn v(k.ty, k.v == RLC_STMT ? k.S : k.N, k.m, k.n, k.p);  // (k.p[0 .. 7] are the slots VI_A .. VI_TH)
  const uint64_t* rho = (const uint64_t*)k.p[RLC_RHO];
  uint8_t* ok = (uint8_t*)k.out(RLC_OK);
  switch (k.v) {
    case RLC_PLAIN:
      return DISPATCH(c, verify_rlc(c, v, rho, k.out(RLC_ACC)));
    case RLC_LOCATE:
      return DISPATCH(c, verify_rlc_locate(c, v, rho, k.out(RLC_ACC), ok, (uint32_t*)k.out(RLC_INFO)));
    case RLC_STMT:
      return DISPATCH(c, verify_stmt_rlc(c, v, k.N, rho, k.out(RLC_ACC), ok));
    case RLC_EQ:
      return DISPATCH(c, verify_eq_rlc(c, v, rho, k.out(RLC_ACC)));
  }
  return GS_ERR_ARG;
}
// Any of the eight: device pointers run as they are; host pointers are staged in, run and the outputs copied back.
// ok_all (gs_verify_batch_rlc and gs_verify_equation_rlc only; may be NULL): gs_gt_finalize on the returned pair.
static int rlc_call(gs_ctx* c, const RlcCall& k, bool host, uint8_t* ok_all = nullptr) {
  RlcArr a[RLC_MAX];
  int na;
  RC(rlc_check(c, k, host, a, &na));
  if (!host) return rlc_run(c, k);
  std::vector<uint8_t> spare[RLC_MAX];  // an optional output the caller left out is still written: it lands here
  for (int i = 0; i < na; i++)
    if (!a[i].p) {
      spare[i].resize(a[i].bytes);
      a[i].p = spare[i].data();
    }
  HostStage st(c);
  RlcCall d = k;
  for (int i = 0; i < na; i++) {
    void* dp;
    RC(a[i].flags & ARR_OUT ? st.out(const_cast<void*>(a[i].p), a[i].bytes, &dp) : st.in(a[i].p, a[i].bytes, &dp));
    d.p[i] = dp;
  }
  RC(rlc_run(c, d));
  for (int i = 0; i < na; i++)
    if (a[i].flags & ARR_OUT) RC(st.back(const_cast<void*>(a[i].p), d.p[i], a[i].bytes));
  if (ok_all) RC(gs_gt_finalize(c, 1, a[RLC_ACC].p, ok_all));
  return GS_OK;
}
int gs_verify_batch_rlc_dev(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G,
                            const void* target, const void* xcoms, const void* ycoms, const void* pi,
                            const void* theta, const uint64_t* rho, void* acc) {
  return rlc_call(c, {RLC_PLAIN, ty, 1, N, m, n, {A, B, G, target, xcoms, ycoms, pi, theta, rho, acc}}, false);
}
int gs_verify_batch_rlc(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G,
                        const void* target, const void* xcoms, const void* ycoms, const void* pi, const void* theta,
                        const uint64_t* rho, void* acc, uint8_t* ok_all) {
  return rlc_call(c, {RLC_PLAIN, ty, 1, N, m, n, {A, B, G, target, xcoms, ycoms, pi, theta, rho, acc}}, true, ok_all);
}
// ---- batched verifier with fault localisation: the product tree is kept and descended from the root ----------------
int gs_verify_batch_rlc_locate_dev(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G,
                                   const void* target, const void* xcoms, const void* ycoms, const void* pi,
                                   const void* theta, const uint64_t* rho, void* acc, uint8_t* ok, uint32_t* info) {
  return rlc_call(c, {RLC_LOCATE, ty, 1, N, m, n, {A, B, G, target, xcoms, ycoms, pi, theta, rho, acc, ok, info}}, false);
}
int gs_verify_batch_rlc_locate(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G,
                               const void* target, const void* xcoms, const void* ycoms, const void* pi,
                               const void* theta, const uint64_t* rho, void* acc, uint8_t* ok, uint32_t* info) {
  return rlc_call(c, {RLC_LOCATE, ty, 1, N, m, n, {A, B, G, target, xcoms, ycoms, pi, theta, rho, acc, ok, info}}, true);
}
// statement-batched: S statements of E equations over shared commitments
int gs_verify_statements_rlc_dev(gs_ctx* c, int ty, size_t S, size_t E, int m, int n, const void* A, const void* B,
                                 const void* G, const void* target, const void* xcoms, const void* ycoms, const void* pi,
                                 const void* theta, const uint64_t* rho, void* acc, uint8_t* ok) {
  return rlc_call(c, {RLC_STMT, ty, S, E, m, n, {A, B, G, target, xcoms, ycoms, pi, theta, rho, acc, ok}}, false);
}
int gs_verify_statements_rlc(gs_ctx* c, int ty, size_t S, size_t E, int m, int n, const void* A, const void* B,
                             const void* G, const void* target, const void* xcoms, const void* ycoms, const void* pi,
                             const void* theta, const uint64_t* rho, void* acc, uint8_t* ok) {
  return rlc_call(c, {RLC_STMT, ty, S, E, m, n, {A, B, G, target, xcoms, ycoms, pi, theta, rho, acc, ok}}, true);
}
// N proofs of ONE equation: the constants are one copy, the combination is taken across the proofs before pairing
int gs_verify_equation_rlc_dev(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G,
                               const void* target, const void* xcoms, const void* ycoms, const void* pi,
                               const void* theta, const uint64_t* rho, void* acc) {
  return rlc_call(c, {RLC_EQ, ty, 1, N, m, n, {A, B, G, target, xcoms, ycoms, pi, theta, rho, acc}}, false);
}
int gs_verify_equation_rlc(gs_ctx* c, int ty, size_t N, int m, int n, const void* A, const void* B, const void* G,
                           const void* target, const void* xcoms, const void* ycoms, const void* pi, const void* theta,
                           const uint64_t* rho, void* acc, uint8_t* ok_all) {
  return rlc_call(c, {RLC_EQ, ty, 1, N, m, n, {A, B, G, target, xcoms, ycoms, pi, theta, rho, acc}}, true, ok_all);
}
int gs_gt_finalize_dev(gs_ctx* c, size_t count, const void* accs_dev, uint8_t* ok) {
  RC(check_ctx(c, false));
  if (!accs_dev || !ok || count == 0) return fail(c, GS_ERR_ARG, "null pointer");
  return DISPATCH(c, gt_finalize(c, count, accs_dev, ok, true));
}
int gs_gt_finalize(gs_ctx* c, size_t count, const void* accs, uint8_t* ok) {
  RC(check_ctx(c, false));
  if (!accs || !ok || count == 0) return fail(c, GS_ERR_ARG, "null pointer");
  return DISPATCH(c, gt_finalize(c, count, accs, ok));
}

// ---- profiling ---------------------------------------------------------------------


int gs_wire_sizes(int curve, size_t out[6]) {
  if ((curve != 0 && curve != 1) || !out) return GS_ERR_ARG;
  size_t fq = sz_fq(curve);
  out[0] = fq;       // G1 compressed
  out[1] = 2 * fq;   // G1 uncompressed
  out[2] = 2 * fq;   // G2 compressed
  out[3] = 4 * fq;   // G2 uncompressed
  out[4] = SZ_FR;    // Fr
  out[5] = 12 * fq;  // GT
  return GS_OK;
}
int gs_wire_encode_g1(gs_ctx* c, size_t n, int compressed, const void* pts, uint8_t* out) {
  RC(check_ctx(c, false));
  return WIRE_DISPATCH((WireImpl<Bls12_381>::enc_pts<Fq<Bls12_381>>(c, n, compressed, pts, out)),
                       (WireImpl<Bn254>::enc_pts<Fq<Bn254>>(c, n, compressed, pts, out)));
}
int gs_wire_encode_g2(gs_ctx* c, size_t n, int compressed, const void* pts, uint8_t* out) {
  RC(check_ctx(c, false));
  return WIRE_DISPATCH((WireImpl<Bls12_381>::enc_pts<Fp2<Bls12_381>>(c, n, compressed, pts, out)),
                       (WireImpl<Bn254>::enc_pts<Fp2<Bn254>>(c, n, compressed, pts, out)));
}
int gs_wire_decode_g1(gs_ctx* c, size_t n, int compressed, int validate, const uint8_t* in, void* pts, uint8_t* ok) {
  RC(check_ctx(c, false));
  return WIRE_DISPATCH((WireImpl<Bls12_381>::dec_pts<Fq<Bls12_381>>(c, n, compressed, validate, in, pts, ok)),
                       (WireImpl<Bn254>::dec_pts<Fq<Bn254>>(c, n, compressed, validate, in, pts, ok)));
}
int gs_wire_decode_g2(gs_ctx* c, size_t n, int compressed, int validate, const uint8_t* in, void* pts, uint8_t* ok) {
  RC(check_ctx(c, false));
  return WIRE_DISPATCH((WireImpl<Bls12_381>::dec_pts<Fp2<Bls12_381>>(c, n, compressed, validate, in, pts, ok)),
                       (WireImpl<Bn254>::dec_pts<Fp2<Bn254>>(c, n, compressed, validate, in, pts, ok)));
}
// ---- subgroup safety at the boundary ------------------------------------------------------
int gs_validate_points_dev(gs_ctx* c, int group, size_t n, const void* pts, uint8_t* ok) {
  RC(check_ctx(c, false));
  if (group != 1 && group != 2) return fail(c, GS_ERR_ARG, "group: 1 (G1) or 2 (G2)");
  if (n == 0) return GS_OK;
  if (!pts || !ok) return fail(c, GS_ERR_ARG, "null pointer");
  if (c->curve == 0)
    return group == 1 ? WireImpl<Bls12_381>::validate_pts_dev<Fq<Bls12_381>>(c, n, pts, ok)
                      : WireImpl<Bls12_381>::validate_pts_dev<Fp2<Bls12_381>>(c, n, pts, ok);
  return group == 1 ? WireImpl<Bn254>::validate_pts_dev<Fq<Bn254>>(c, n, pts, ok)
                    : WireImpl<Bn254>::validate_pts_dev<Fp2<Bn254>>(c, n, pts, ok);
}
int gs_validate_points(gs_ctx* c, int group, size_t n, const void* pts, uint8_t* ok) {
  RC(check_ctx(c, false));
  if (group != 1 && group != 2) return fail(c, GS_ERR_ARG, "group: 1 (G1) or 2 (G2)");
  if (n == 0) return GS_OK;
  if (!pts || !ok) return fail(c, GS_ERR_ARG, "null pointer");
  const size_t pb = (group == 1 ? 2 : 4) * sz_fq(c->curve);
  return staged_call(c, {{pts, n * pb}}, {{ok, n}},
                     [&](void** d) { return gs_validate_points_dev(c, group, n, d[0], (uint8_t*)d[1]); });
}

int gs_wire_encode_fr(gs_ctx* c, size_t n, const void* fr, uint8_t* out) {
  RC(check_ctx(c, false));
  return WIRE_DISPATCH(WireImpl<Bls12_381>::fields(c, 0, 0, 0, n, fr, out, nullptr),
                       WireImpl<Bn254>::fields(c, 0, 0, 0, n, fr, out, nullptr));
}
int gs_wire_decode_fr(gs_ctx* c, size_t n, const uint8_t* in, void* fr, uint8_t* ok) {
  RC(check_ctx(c, false));
  if (!ok) return GS_ERR_ARG;
  return WIRE_DISPATCH(WireImpl<Bls12_381>::fields(c, 0, 1, 0, n, in, fr, ok),
                       WireImpl<Bn254>::fields(c, 0, 1, 0, n, in, fr, ok));
}
int gs_wire_encode_gt(gs_ctx* c, size_t n, const void* gt, uint8_t* out) {
  RC(check_ctx(c, false));
  return WIRE_DISPATCH(WireImpl<Bls12_381>::fields(c, 1, 0, 0, n, gt, out, nullptr),
                       WireImpl<Bn254>::fields(c, 1, 0, 0, n, gt, out, nullptr));
}
int gs_wire_decode_gt(gs_ctx* c, size_t n, int validate, const uint8_t* in, void* gt, uint8_t* ok) {
  RC(check_ctx(c, false));
  if (!ok) return GS_ERR_ARG;
  return WIRE_DISPATCH(WireImpl<Bls12_381>::fields(c, 1, 1, validate, n, in, gt, ok),
                       WireImpl<Bn254>::fields(c, 1, 1, validate, n, in, gt, ok));
}

#if defined(GS_DEBUG_STAMPS)
// diagnosis build only: read and clear the phase stamps of the G1 / G2 Straus lanes (gs_curve.cuh, gs_dbg)
int gs_debug_stamps(gs_ctx* c, unsigned long long* out16) {
  RC(check_ctx(c, false));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyFromSymbol(out16, HIP_SYMBOL(gs::gs_dbg), 16 * sizeof(unsigned long long)));
  unsigned long long z[16] = {0};
  HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(gs::gs_dbg), z, sizeof z));
  return GS_OK;
}
#endif
int gs_prof_enable(gs_ctx* c, int on) {
  if (!c) return GS_ERR_ARG;
  c->prof = on != 0;
  return GS_OK;
}
int gs_prof_reset(gs_ctx* c) {
  if (!c) return GS_ERR_ARG;
  c->prof_map.clear();
  c->prof_order.clear();
  return GS_OK;
}
int gs_prof_get(gs_ctx* c, int idx, char* name, size_t cap, double* ms, uint64_t* n) {
  if (!c || idx < 0 || (size_t)idx >= c->prof_order.size()) return GS_ERR_ARG;
  const std::string& k = c->prof_order[idx];
  if (name && cap) {
    strncpy(name, k.c_str(), cap - 1);
    name[cap - 1] = 0;
  }
  if (ms) *ms = c->prof_map[k].ms;
  if (n) *n = c->prof_map[k].n;
  return GS_OK;
}
// clock (GHz) the launches under entry idx ran at: sum over their waves of d s_memtime / d s_memrealtime x 100 MHz, taken
// inside those very launches (k_seg stamps); 0 for kernels that are not segmented launches
int gs_prof_get_clock(gs_ctx* c, int idx, double* ghz) {
  if (!c || !ghz || idx < 0 || idx >= (int)c->prof_order.size()) return GS_ERR_ARG;
  const ProfEntry& p = c->prof_map[c->prof_order[idx]];
  *ghz = p.rt > 0 ? p.cyc / p.rt * 0.1 : 0.0;
  return GS_OK;
}
int gs_prof_get_work(gs_ctx* c, int idx, uint64_t* lanes, uint64_t* work) {
  if (!c || idx < 0 || (size_t)idx >= c->prof_order.size()) return GS_ERR_ARG;
  const ProfEntry& p = c->prof_map[c->prof_order[idx]];
  if (lanes) *lanes = p.lanes;
  if (work) *work = p.work;
  return GS_OK;
}

}  // extern "C"
