// Step executor: the hot path of one tile (K1+K2 -> slot reduction + solve -> K3) as PREPARED launches, and the
// one-tile-deep pipeline of SpectralFusion.submit() (fit of tile i on a side stream under K1 of tile i+1) with its HIP
// events and stream waits issued from C.
//
// Why (profiles/r03_strong_scaling.md): a rank of an 8-way strong-scaling run processes a 128 x 1024 row block per step -
// 36 us of GPU work in the pipelined order - while the Python side of submit() (argument marshalling of three ctypes
// calls with 15-25 arguments each, two torch stream contexts, four event operations) takes ~60 us: host bound.  A plan
// stores every argument once; running a step is one call with the three pointers that change from tile to tile.
// The kernels are the ones behind hsr_srf_integrate_moments / hsr_moments_reduce[_solve] / hsr_poly_solve /
// hsr_poly_apply: same launches, same bits.
#include <new>
#include <vector>

#include "hsr_common.h"
#include "hsr_solve.h"
#include "hsr_sync_dev.h"
#include "hsr_fused_dev.h"

// The prepared launches of one tile and nothing else: creating a plan makes no HIP call.
struct hsr_step_plan {
  hsr_step_desc d;
  int32_t k0[HSR_MAX_BANDS], klen[HSR_MAX_BANDS];
  int32_t slots;                  // partial slots of the last K1 launch
};

enum { kTwoSlot = 0, kFused = 1, kExchange = 2, kGroup = 3 };
enum { kSyncDrainTickets = 8, kSyncWords = 12 };   // hsr_pipeline.sync

// One slot of a pipeline: the plan it launches and the state of the tile it holds.
struct pipe_slot {
  hsr_step_plan* p = nullptr;
  hipEvent_t ev_k1 = nullptr;     // two slots: K1 of this slot's tile enqueued
  hipEvent_t ev_fit = nullptr;    // two slots, exchange: fit of this slot's tile done
  bool pending = false;           // K1 + fit enqueued, K3 not yet
  bool fitted = false;            // fused forms: the slot reduction (+ solve, without an exchange) of this slot's tile has been enqueued
  bool exchanged = false;         // exchange: gate -> collective -> solve of this slot's tile has been enqueued on the side stream
  unsigned int seq = 0;           // exchange: sequence number of the tile in this slot (the value of its "ready" word)
};

struct hsr_pipeline {
  std::vector<pipe_slot> slot;
  int kind = kTwoSlot;            // kTwoSlot: K3(i-1) as its own launch behind K1(i);  kFused (3 slots): K3(i-2) inside K1(i)'s launch;
                                  // kExchange (4 slots): K3(i-3) inside K1(i)'s launch, exchange issued from C (hsr_pipeline_create_exchange);
                                  // kGroup (T + 2 slots): one fit per group of T tiles, K3(i-T-1) inside K1(i)'s launch (hsr_pipeline_create_group)
  int nslots = 0;
  int group_T = 0;                // kGroup: tiles per fit
  double* group_moments = nullptr;  // kGroup: [2][T][nb][M] per-tile moments, by group parity
  double* group_total = nullptr;    //         [2][nb][M]
  double* group_coeffs = nullptr;   //         [2][nb][deg+1]
  hipStream_t side = nullptr;
  int64_t n = 0;                  // tiles submitted
  int exchange = 0;               // two slots, 1: the caller runs the fit (reduce -> collective -> solve) itself between
                                  //    hsr_pipeline_submit and hsr_pipeline_fit_done
  unsigned int* sync = nullptr;   // fused forms, device words: [0] ticket counter of the tail fits, [1] bands whose moments are published,
                                  //   [2] error code, [4 + k] "coefficients ready" word of slot k (holds the sequence number of its tile),
                                  //   [8] ticket counter of the drain launches (three slots)
  unsigned int tickets = 0;       // value sync[0] reaches once every launch enqueued so far has run
  unsigned int drain_tickets = 0; // the same for sync[8]
  // ---- four slots: the exchange is issued from here ----
  hsr_exchange x{};
  unsigned int published = 0;     // value sync[1] reaches once every reduction enqueued so far has run (nb per tile)
  int deferred = -1;              // slot whose solve + publish is not enqueued yet: it rides in the launch that gates the NEXT tile's
  int deferred_solve = 0;         // collective (one side-stream launch per step instead of two), or goes out alone at a drain; -1: none
  double* host_moments[4] = {};   // pinned staging of the host_sum transport, one per slot
  struct host_job { hsr_pipeline* pl; double* values; int32_t count; } host_jobs[4] = {};
  volatile int host_error = 0;    // host_sum returned non-zero
};

namespace {

// ---- kernels of the exchange pipeline (four slots) ----------------------------------------------------------------
// gate: one wave on the side stream that polls a device word until it has reached `target` - the stream-ordered work behind
// it (the collective, the solve) then starts without any event on the caller's stream.  1 wave, no LDS, a handful of
// registers: it fits on a CU the persistent K1 leaves free (hsr_srf_options.reserved_cus).
__global__ __launch_bounds__(64) void gate_kernel(const unsigned int* word, unsigned int target, unsigned int* err, unsigned int code) {
  if (threadIdx.x == 0) hsr::wait_word_at_least(word, target, err, code);
}

// adds `n` to a word at agent scope: tiles whose slot reduction ran as a launch of its own publish their moments this way
__global__ __launch_bounds__(64) void publish_add_kernel(unsigned int* word, unsigned int n) {
  if (threadIdx.x == 0) __hip_atomic_fetch_add(word, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Rehearsal stand-in for the collective's kernel on a one-GPU box (hsr_exchange.rehearsal_us): resident for `us` microseconds with
// the footprint of a small RCCL kernel, computes nothing.
__global__ __launch_bounds__(256) void rehearsal_collective_kernel(int us, unsigned int* sink) {
  __shared__ unsigned int lds[12288];          // 48 KB
  lds[threadIdx.x] = threadIdx.x;
  __syncthreads();
  const unsigned long long t0 = hsr::sync_realtime();
  while (hsr::sync_realtime() - t0 < (unsigned long long)us * 100ull) __builtin_amdgcn_s_sleep(8);
  if (lds[(threadIdx.x * 7) & 255] == 0xffffffffu) *sink = 1u;      // never true: keeps the LDS allocation
}

// np.polyfit from the (all-reduced) moments, one thread per band - solve_kernel of hsr_poly.hip, hence its bits - and then the
// publication: coefficients written through to memory, stores waited for, the slot's "ready" word set to the tile's sequence
// number.  do_solve = 0: publish only (the coefficients came by broadcast).
// gate_word != NULL: the kernel then goes on as the NEXT tile's gate (one launch per step on the side stream instead of two).
__global__ __launch_bounds__(64) void solve_publish_kernel(const double* __restrict__ moments, int nb, int deg, long long min_count,
                                                           double* coeffs, int do_solve, unsigned int* ready, unsigned int value,
                                                           const unsigned int* gate_word, unsigned int gate_target, unsigned int* err) {
  const int b = threadIdx.x;
  if (do_solve && b < nb) {
    double c[HSR_MAX_DEG + 1];
    hsr::solve_band(moments + (size_t)b * hsr::moment_count(deg), deg, min_count, c);
    for (int j = 0; j <= deg; ++j)
      __hip_atomic_store(coeffs + (size_t)b * (deg + 1) + j, c[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    hsr::st_agent_u32(ready, value);
    if (gate_word) hsr::wait_word_at_least(gate_word, gate_target, err, 1u);
  }
}

// ---- drain of the three-slot fused pipeline ----------------------------------------------------------------------------
// When no further K1 launch comes, the two ends of a carrying launch still go out as ONE kernel: K3 of the older pending tile as the
// body (apply_prephase: the bits of apply_rows_kernel), the fit of the newest tile as the tail (lazy_fit: the bits of
// hsr_moments_reduce_solve), by tickets of a counter of its own.  Both read what EARLIER launches wrote, so nothing crosses between
// running workgroups and nothing is waited for; the newest tile's own K3 stays behind the launch boundary.  Needs gridDim.x >= nb
// like every launch with a tail fit.  No exchange, no group fit: those members are fixed, the branches behind them compiled out.
// (In this file, not next to the K1 kernels: a further caller of solve_band_t in their translation unit changed their register
// allocation - the degree-3 instances went from 48 to 96 bytes of private segment.)
struct DrainArgs {
  int32_t nb;
  int64_t out_ps;
  const float* apply_x;
  float* apply_out;
  const double* apply_coeffs;
  const uint8_t* apply_mask;
  int64_t apply_npix;
  int32_t apply_clip;
  const double* lazy_partials;
  int32_t lazy_slots;
  long long lazy_min_count;
  double* lazy_moments;
  double* lazy_coeffs;
  unsigned int* lazy_counter;
  unsigned int lazy_base;
  unsigned int* lazy_ready;         // always NULL here (a compile-time NULL trips -Wnonnull in the atomic of the dead branch)
  static constexpr const unsigned int* apply_ready = nullptr;
  static constexpr unsigned int apply_ready_value = 0;
  static constexpr unsigned int* sync_error = nullptr;
  static constexpr int32_t lazy_group_T = 0, lazy_group_index = 0;
  static constexpr const double* lazy_group_moments = nullptr;
  static constexpr double* lazy_group_total = nullptr;
};
constexpr int kDrainThreads = 512;
constexpr int kDrainLds = 64 + 64 * 16 * 8 + (16 + hsr::kSolveWork + 16) * 8;   // lazy_fit: ticket, lane sums, moments, solve work area
template <int DEG>
__global__ __launch_bounds__(kDrainThreads, 4) void drain_apply_fit_kernel(const DrainArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kDrainLds];
  const int t = threadIdx.x;
  hsr::apply_prephase<DEG + 1, kDrainThreads>(a, smem, t);
  hsr::lazy_fit<DEG, kDrainThreads>(a, smem, t);
}

int run_drain(const hsr_apply_job& job, const hsr_step_desc& d, int grid, hipStream_t stream) {
  const char* who = "hsr_pipeline_flush (drain)";
  HSR_REQUIRE(job.x_dev && job.out_dev && job.coeffs_dev && job.npix >= 1 && job.fit_partials_dev && job.fit_moments_dev &&
                  job.fit_coeffs_dev && job.fit_counter_dev && job.fit_slots >= 1 && job.fit_min_count >= 0,
              HSR_ERR_INVALID, "%s: NULL pointer, npix < 1 or an incomplete tail fit", who);
  // (hsr_pipeline_create_fused has checked the rows: 16-byte aligned, pixel-major, 4 / 8 / 12 / 16 floats)
  HSR_REQUIRE(job.npix * (d.out_ps >> 2) < ((int64_t)1 << 31), HSR_ERR_UNSUPPORTED, "%s: %lld pixels of %lld floats exceed 2^31 float4",
              who, (long long)job.npix, (long long)d.out_ps);
  // one ticket per workgroup, one band per ticket
  HSR_REQUIRE(grid >= d.nb && grid <= 512, HSR_ERR_UNSUPPORTED, "%s: %d workgroups cannot fit %d bands", who, grid, d.nb);
  DrainArgs a{};
  a.nb = d.nb;
  a.out_ps = d.out_ps;
  a.apply_x = job.x_dev;
  a.apply_out = job.out_dev;
  a.apply_coeffs = job.coeffs_dev;
  a.apply_mask = job.mask_dev;
  a.apply_npix = job.npix;
  a.apply_clip = job.clip;
  a.lazy_partials = job.fit_partials_dev;
  a.lazy_slots = job.fit_slots;
  a.lazy_min_count = (long long)job.fit_min_count;
  a.lazy_moments = job.fit_moments_dev;
  a.lazy_coeffs = job.fit_coeffs_dev;
  a.lazy_counter = job.fit_counter_dev;
  a.lazy_base = job.fit_ticket_base;
  switch (d.deg) {
    case 1: hipLaunchKernelGGL(drain_apply_fit_kernel<1>, dim3(grid), dim3(kDrainThreads), 0, stream, a); break;
    case 2: hipLaunchKernelGGL(drain_apply_fit_kernel<2>, dim3(grid), dim3(kDrainThreads), 0, stream, a); break;
    case 3: hipLaunchKernelGGL(drain_apply_fit_kernel<3>, dim3(grid), dim3(kDrainThreads), 0, stream, a); break;
    case 4: hipLaunchKernelGGL(drain_apply_fit_kernel<4>, dim3(grid), dim3(kDrainThreads), 0, stream, a); break;
    default: HSR_REQUIRE(false, HSR_ERR_UNSUPPORTED, "%s: deg=%d", who, d.deg);
  }
  HSR_LAUNCH_CHECK("drain_apply_fit_kernel");
  return HSR_OK;
}

int run_k1(hsr_step_plan* p, const void* cube, const float* real, const uint8_t* mask, hipStream_t s,
           const hsr_apply_job* job = nullptr) {
  const hsr_step_desc& d = p->d;
  if (job && d.cube_dtype == 2)
    return hsr_srf_integrate_moments_u16_apply(static_cast<const uint16_t*>(cube), d.npix, d.B, d.scale, d.nodata, d.wn_dev, p->k0,
                                               p->klen, d.nb, d.pseudo_dev, d.out_bs, d.out_ps, real, d.real_bs, d.real_ps, mask,
                                               d.min_x, d.min_y, d.deg, d.partials_dev, &p->slots, &d.opts, job, s);
  if (job)
    return hsr_srf_integrate_moments_apply(static_cast<const float*>(cube), d.npix, d.B, d.wn_dev, p->k0, p->klen, d.nb,
                                           d.pseudo_dev, d.out_bs, d.out_ps, real, d.real_bs, d.real_ps, mask, d.min_x, d.min_y,
                                           d.deg, d.partials_dev, &p->slots, &d.opts, job, s);
  if (d.cube_dtype == 2)
    return hsr_srf_integrate_moments_u16(static_cast<const uint16_t*>(cube), d.npix, d.B, d.scale, d.nodata, d.wn_dev, p->k0,
                                         p->klen, d.nb, d.pseudo_dev, d.out_bs, d.out_ps, real, d.real_bs, d.real_ps, mask,
                                         d.min_x, d.min_y, d.deg, d.partials_dev, &p->slots, &d.opts, s);
  return hsr_srf_integrate_moments(static_cast<const float*>(cube), d.npix, d.B, d.wn_dev, p->k0, p->klen, d.nb, d.pseudo_dev,
                                   d.out_bs, d.out_ps, real, d.real_bs, d.real_ps, mask, d.min_x, d.min_y, d.deg,
                                   d.partials_dev, &p->slots, &d.opts, s);
}

// K1 with the caller's timing events (either may be NULL) bound to the dispatch: they bracket exactly this launch and put no marker
// packet on the stream (two hipEventRecord calls round a launch cost ~12 us of launch gap).
int run_k1_timed(hsr_step_plan* p, const void* cube, const float* real, const uint8_t* mask, hipStream_t s, const hsr_apply_job* job,
                 void* begin_event, void* end_event) {
  hsr::srf_bind_launch_events((hipEvent_t)begin_event, (hipEvent_t)end_event);
  const int rc = run_k1(p, cube, real, mask, s, job);
  hsr::srf_bind_launch_events(nullptr, nullptr);      // (a call that failed before its launch leaves the record behind)
  return rc;
}

int run_apply(const hsr_step_plan* p, const double* coeffs, const uint8_t* mask, hipStream_t s) {
  const hsr_step_desc& d = p->d;
  return hsr_poly_apply(d.pseudo_dev, d.out_bs, d.out_ps, d.apply_mask ? mask : nullptr, coeffs, d.nb, d.deg, d.npix,
                        nullptr, d.clip, d.matched_dev, d.matched_bs, d.matched_ps, s);
}

}  // namespace

extern "C" int hsr_step_plan_create(const hsr_step_desc* desc, hsr_step_plan** out) {
  HSR_REQUIRE(desc && out, HSR_ERR_INVALID, "hsr_step_plan_create: NULL argument");
  HSR_REQUIRE(desc->nb >= 1 && desc->nb <= HSR_MAX_BANDS && desc->k0 && desc->klen, HSR_ERR_INVALID,
              "hsr_step_plan_create: nb=%d outside [1,%d] or NULL band tables", desc->nb, HSR_MAX_BANDS);
  HSR_REQUIRE(desc->deg >= 1 && desc->deg <= HSR_MAX_DEG, HSR_ERR_INVALID, "hsr_step_plan_create: deg=%d outside [1,%d]",
              desc->deg, HSR_MAX_DEG);
  HSR_REQUIRE(desc->cube_dtype == 0 || desc->cube_dtype == 2, HSR_ERR_INVALID, "hsr_step_plan_create: cube_dtype %d (0 float32, 2 uint16)",
              desc->cube_dtype);
  HSR_REQUIRE(desc->npix >= 1 && desc->wn_dev && desc->pseudo_dev && desc->matched_dev && desc->partials_dev && desc->moments_dev &&
                  desc->coeffs_dev, HSR_ERR_INVALID, "hsr_step_plan_create: NULL device pointer or npix < 1");
  hsr_step_plan* p = new (std::nothrow) hsr_step_plan();
  HSR_REQUIRE(p, HSR_ERR_INVALID, "hsr_step_plan_create: out of host memory");
  p->d = *desc;
  for (int b = 0; b < desc->nb; ++b) {
    p->k0[b] = desc->k0[b];
    p->klen[b] = desc->klen[b];
  }
  p->d.k0 = p->k0;          // the plan owns its copy of the host tables
  p->d.klen = p->klen;
  *out = p;
  return HSR_OK;
}

extern "C" void hsr_step_plan_destroy(hsr_step_plan* p) { delete p; }

extern "C" int hsr_step_plan_slots(const hsr_step_plan* p) { return p ? p->slots : -1; }


extern "C" int hsr_step_run(hsr_step_plan* p, const void* cube_dev, const float* real_dev, const uint8_t* mask_dev,
                            hsr_stream_t stream) {
  HSR_REQUIRE(p && cube_dev && real_dev, HSR_ERR_INVALID, "hsr_step_run: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  int rc = run_k1(p, cube_dev, real_dev, mask_dev, s);
  if (rc != HSR_OK) return rc;
  rc = hsr_moments_reduce_solve(p->d.partials_dev, p->slots, p->d.nb, p->d.deg, p->d.min_count, p->d.moments_dev, p->d.coeffs_dev, s);
  if (rc != HSR_OK) return rc;
  return run_apply(p, p->d.coeffs_dev, mask_dev, s);
}

extern "C" int hsr_step_run_k1(hsr_step_plan* p, const void* cube_dev, const float* real_dev, const uint8_t* mask_dev,
                               hsr_stream_t stream) {
  HSR_REQUIRE(p && cube_dev && real_dev, HSR_ERR_INVALID, "hsr_step_run_k1: NULL argument");
  return run_k1(p, cube_dev, real_dev, mask_dev, (hipStream_t)stream);
}

extern "C" int hsr_step_run_reduce(hsr_step_plan* p, hsr_stream_t stream) {
  HSR_REQUIRE(p, HSR_ERR_INVALID, "hsr_step_run_reduce: NULL plan");
  return hsr_moments_reduce(p->d.partials_dev, p->slots, p->d.nb, p->d.deg, p->d.moments_dev, stream);
}

extern "C" int hsr_step_run_solve(hsr_step_plan* p, hsr_stream_t stream) {
  HSR_REQUIRE(p, HSR_ERR_INVALID, "hsr_step_run_solve: NULL plan");
  return hsr_poly_solve(p->d.moments_dev, p->d.nb, p->d.deg, p->d.min_count, p->d.coeffs_dev, stream);
}

extern "C" int hsr_step_run_apply(hsr_step_plan* p, const uint8_t* mask_dev, hsr_stream_t stream) {
  HSR_REQUIRE(p, HSR_ERR_INVALID, "hsr_step_run_apply: NULL plan");
  return run_apply(p, p->d.coeffs_dev, mask_dev, (hipStream_t)stream);
}

// ---- pipeline ------------------------------------------------------------------------------------------------
//     caller's stream :  K1(0)  K1(1)  K3(0)  K1(2)  K3(1)  ...
//     side stream     :  fit(0)        fit(1)        fit(2) ...          fit(i) runs under K1(i+1)
// K3(i) waits for ev_fit(i) and precedes K1(i+2) in stream order, so two slots need no further events.  The event that
// releases fit(i) is recorded behind K3(i-1), not between K1(i) and K3(i-1) (a record in between cost a 13 us bubble).
// Argument checks first, then the HIP objects of the form: the device words of the fused forms, the events of the forms with
// side-stream work (two slots, exchange).
static int pipeline_new(hsr_step_plan* const* sl, int nslots, int kind, hsr_stream_t side_stream, hsr_pipeline** out, const char* who) {
  HSR_REQUIRE(out, HSR_ERR_INVALID, "%s: NULL argument", who);
  for (int i = 0; i < nslots; ++i) {
    HSR_REQUIRE(sl[i], HSR_ERR_INVALID, "%s: NULL plan", who);
    for (int k = 0; k < i; ++k) {
      HSR_REQUIRE(sl[i] != sl[k], HSR_ERR_INVALID, "%s: distinct plans needed", who);
      // In one fused launch the pre-phase reads the coefficients of one slot, the tail writes the moments / coefficients and reads
      // the partials of another, K1 writes the partials of a third: aliased work buffers would race silently.
      const hsr_step_desc &a = sl[i]->d, &b = sl[k]->d;
      HSR_REQUIRE(kind == kTwoSlot || (a.partials_dev != b.partials_dev && a.moments_dev != b.moments_dev && a.coeffs_dev != b.coeffs_dev &&
                                       a.pseudo_dev != b.pseudo_dev && a.matched_dev != b.matched_dev),
                  HSR_ERR_INVALID, "%s: plans %d and %d share a work buffer (partials / moments / coefficients / images must be distinct)", who, k, i);
    }
  }
  HSR_REQUIRE(side_stream != nullptr, HSR_ERR_INVALID, "%s: the side stream must be a real stream, not the default one", who);
  hsr_pipeline* pl = new (std::nothrow) hsr_pipeline();
  HSR_REQUIRE(pl, HSR_ERR_INVALID, "%s: out of host memory", who);
  pl->slot.resize(nslots);
  for (int k = 0; k < nslots; ++k) pl->slot[k].p = sl[k];
  pl->kind = kind;
  pl->nslots = nslots;
  pl->side = (hipStream_t)side_stream;
  bool ok = true;
  if (kind != kTwoSlot)           // not a launch-path call
    ok = hipMalloc(&pl->sync, kSyncWords * sizeof(unsigned int)) == hipSuccess && hipMemset(pl->sync, 0, kSyncWords * sizeof(unsigned int)) == hipSuccess &&
         hipDeviceSynchronize() == hipSuccess;
  if (kind == kTwoSlot || kind == kExchange)
    for (pipe_slot& s : pl->slot)
      ok = ok && hipEventCreateWithFlags(&s.ev_fit, hipEventDisableTiming) == hipSuccess &&
           (kind != kTwoSlot || hipEventCreateWithFlags(&s.ev_k1, hipEventDisableTiming) == hipSuccess);
  if (!ok) {
    (void)hipGetLastError();
    hsr_pipeline_destroy(pl);
    hsr::set_error("%s: could not create the pipeline's device words or events", who);
    return HSR_ERR_HIP;
  }
  *out = pl;
  return HSR_OK;
}

extern "C" int hsr_pipeline_create(hsr_step_plan* slot0, hsr_step_plan* slot1, hsr_stream_t side_stream, int32_t exchange,
                                   hsr_pipeline** out) {
  hsr_step_plan* sl[2] = {slot0, slot1};
  int rc = pipeline_new(sl, 2, kTwoSlot, side_stream, out, "hsr_pipeline_create");
  if (rc == HSR_OK) (*out)->exchange = exchange ? 1 : 0;
  return rc;
}

// The fused launches need one tile geometry in every plan, 16-byte aligned pixel-major rows of 4 / 8 / 12 / 16 floats, and a K1
// kernel that can carry the job (hsr_srf_fused_launch_supported: weights in LDS, for uint16 tiles the ring kernel) - checked HERE
// so that a caller can fall back to the two-slot pipeline before any tile is in flight, not at the first carrying launch.
static int fused_geometry(hsr_step_plan* const* ps, int n, const char* who) {
  for (int i = 0; i < n; ++i) {
    HSR_REQUIRE(ps[i], HSR_ERR_INVALID, "%s: NULL plan", who);
    const hsr_step_desc &d = ps[i]->d, &d0 = ps[0]->d;
    HSR_REQUIRE(d.cube_dtype == d0.cube_dtype && d.out_bs == 1 && (d.out_ps & 3) == 0 && d.out_ps <= HSR_MAX_BANDS && d.matched_bs == 1 &&
                    d.matched_ps == d.out_ps && ((((uintptr_t)d.pseudo_dev) | ((uintptr_t)d.matched_dev)) & 15) == 0 &&
                    d.npix == d0.npix && d.out_ps == d0.out_ps && d.nb == d0.nb && d.deg == d0.deg && d.B == d0.B &&
                    d.opts.reserved_cus == d0.opts.reserved_cus,
                HSR_ERR_UNSUPPORTED, "%s: 16-byte aligned pixel-major rows of 4 / 8 / 12 / 16 floats, "
                "the same geometry, cube type and options in all plans", who);
  }
  const hsr_step_desc& d = ps[0]->d;
  return hsr_srf_fused_launch_supported(d.cube_dtype, d.B, d.nb, ps[0]->k0, ps[0]->klen, d.out_ps, d.deg, &d.opts);
}

// Fused pipeline over THREE plans: K3 of tile i-2 rides in the launch of K1 of tile i (hsr_srf_integrate_moments_apply), so the
// caller's stream carries ONE kernel per tile:
//     [K1(0)]  [K1(1) + fit(0)]  [K3(0) + K1(2) + fit(1)]  [K3(1) + K1(3) + fit(2)] ...   nothing else: the fit of tile i is tail
//     work of launch i+1 (first workgroups to finish), no side stream, no events, no free CUs
// No exchange (a collective cannot ride in a kernel's tail): with one, hsr_pipeline_create_exchange.
extern "C" int hsr_pipeline_create_fused(hsr_step_plan* slot0, hsr_step_plan* slot1, hsr_step_plan* slot2, hsr_stream_t side_stream,
                                         int32_t exchange, hsr_pipeline** out) {
  HSR_REQUIRE(!exchange, HSR_ERR_UNSUPPORTED, "hsr_pipeline_create_fused: no exchange in the three-slot form; use hsr_pipeline_create_exchange");
  hsr_step_plan* ps[3] = {slot0, slot1, slot2};
  int rc = fused_geometry(ps, 3, "hsr_pipeline_create_fused");
  if (rc != HSR_OK) return rc;
  return pipeline_new(ps, 3, kFused, side_stream, out, "hsr_pipeline_create_fused");
}

extern "C" int hsr_pipeline_create_exchange(hsr_step_plan* const* slots4, hsr_stream_t side_stream, const hsr_exchange* x,
                                            hsr_pipeline** out) {
  const char* who = "hsr_pipeline_create_exchange";
  HSR_REQUIRE(slots4 && x && out, HSR_ERR_INVALID, "%s: NULL argument", who);
  HSR_REQUIRE((x->comm != nullptr) != (x->host_sum != nullptr), HSR_ERR_INVALID, "%s: exactly one of comm and host_sum must be given", who);
  HSR_REQUIRE(x->mode == HSR_SYNC_ALLREDUCE || x->mode == HSR_SYNC_BROADCAST, HSR_ERR_INVALID, "%s: mode %d", who, x->mode);
  HSR_REQUIRE(!x->comm || (x->root >= 0 && x->root < hsr_comm_ranks(x->comm)), HSR_ERR_INVALID, "%s: root %d", who, x->root);
  HSR_REQUIRE(x->rehearsal_us >= 0 && x->rehearsal_us <= 1000 && x->rehearsal_blocks >= 0 && x->rehearsal_blocks <= 64, HSR_ERR_INVALID,
              "%s: rehearsal stand-in of %d us x %d blocks (at most 1000 us, 64 blocks)", who, x->rehearsal_us, x->rehearsal_blocks);
  int rc = fused_geometry(slots4, 4, who);
  if (rc != HSR_OK) return rc;
  // Not a tuning matter: a K1 launch whose pre-phase polls for coefficients holds every CU it runs on while it waits, and the
  // kernels it waits for (the collective, the solve) are dispatched next to it only where an XCD has a completely free CU
  // (measured in round 2).  With fewer free CUs a late peer turns into a wait that only the polls' time limit ends.
  HSR_REQUIRE(slots4[0]->d.opts.reserved_cus >= 8, HSR_ERR_INVALID, "%s: the plans must leave at least 8 CUs free (hsr_srf_options.reserved_cus >= 8, one "
              "per XCD) for the side stream's kernels; got %d", who, slots4[0]->d.opts.reserved_cus);
  hsr_pipeline* pl = nullptr;
  rc = pipeline_new(slots4, 4, kExchange, side_stream, &pl, who);
  if (rc != HSR_OK) return rc;
  pl->x = *x;
  if (x->host_sum) {
    const size_t bytes = (size_t)pl->slot[0].p->d.nb * hsr::moment_count(pl->slot[0].p->d.deg) * sizeof(double);
    for (int k = 0; k < 4; ++k) {
      if (hipHostMalloc(&pl->host_moments[k], bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        hsr_pipeline_destroy(pl);
        hsr::set_error("%s: could not allocate the pinned staging of the host transport", who);
        return HSR_ERR_HIP;
      }
      pl->host_jobs[k] = {pl, pl->host_moments[k], (int32_t)(bytes / sizeof(double))};
    }
  }
  *out = pl;
  return HSR_OK;
}

extern "C" int hsr_pipeline_create_group(hsr_step_plan* const* slots, int32_t nslots, int32_t group_tiles, double* group_moments_dev,
                                         double* group_total_dev, double* group_coeffs_dev, hsr_stream_t side_stream, hsr_pipeline** out) {
  const char* who = "hsr_pipeline_create_group";
  HSR_REQUIRE(slots && out && group_moments_dev && group_total_dev && group_coeffs_dev, HSR_ERR_INVALID, "%s: NULL argument", who);
  HSR_REQUIRE(group_tiles >= 2 && group_tiles <= 64 && nslots == group_tiles + 2, HSR_ERR_INVALID,
              "%s: groups of 2 .. 64 tiles and group_tiles + 2 plans needed (got %d tiles, %d plans)", who, group_tiles, nslots);
  int rc = fused_geometry(slots, nslots, who);
  if (rc != HSR_OK) return rc;
  hsr_pipeline* pl = nullptr;
  rc = pipeline_new(slots, nslots, kGroup, side_stream, &pl, who);
  if (rc != HSR_OK) return rc;
  pl->group_T = group_tiles;
  pl->group_moments = group_moments_dev;
  pl->group_total = group_total_dev;
  pl->group_coeffs = group_coeffs_dev;
  *out = pl;
  return HSR_OK;
}

extern "C" void hsr_pipeline_destroy(hsr_pipeline* pl) {
  if (!pl) return;
  if (pl->kind == kExchange) (void)hipStreamSynchronize(pl->side);      // a host_sum callback may still point at this object
  for (pipe_slot& s : pl->slot) {
    if (s.ev_k1) (void)hipEventDestroy(s.ev_k1);
    if (s.ev_fit) (void)hipEventDestroy(s.ev_fit);
  }
  for (int k = 0; k < 4; ++k)
    if (pl->host_moments[k]) (void)hipHostFree(pl->host_moments[k]);
  if (pl->sync) (void)hipFree(pl->sync);
  delete pl;
}

static inline pipe_slot& slot_of(hsr_pipeline* pl, int64_t tile) { return pl->slot[tile % pl->nslots]; }

// ---- four slots: the exchange issued from here ------------------------------------------------------------------------
static void host_sum_trampoline(void* arg) {
  auto* j = static_cast<hsr_pipeline::host_job*>(arg);
  if (j->pl->x.host_sum(j->pl->x.host_user, j->values, j->count) != 0) j->pl->host_error = 1;
}

// solve + publish of the deferred slot, optionally going on as the gate of the next tile's collective
static int launch_solve_publish(hsr_pipeline* pl, bool with_gate) {
  const pipe_slot& s = pl->slot[pl->deferred];
  const hsr_step_desc& d = s.p->d;
  hipLaunchKernelGGL(solve_publish_kernel, dim3(1), dim3(64), 0, pl->side, d.moments_dev, d.nb, d.deg, (long long)d.min_count, d.coeffs_dev,
                     pl->deferred_solve, pl->sync + 4 + pl->deferred, s.seq, with_gate ? pl->sync + 1 : nullptr, pl->published, pl->sync + 2);
  HSR_LAUNCH_CHECK("solve_publish_kernel");
  pl->deferred = -1;
  return HSR_OK;
}

// gate -> collective -> solve + publish of the tile in slot k, on the side stream.  Called once per tile, in tile order, on every
// rank: the collectives of all ranks line up.  The solve + publish itself is enqueued with the NEXT tile's gate (or by a drain).
static int enqueue_exchange(hsr_pipeline* pl, int k) {
  const hsr_step_desc& d = pl->slot[k].p->d;
  const int64_t nmom = (int64_t)d.nb * hsr::moment_count(d.deg);
  int rc = HSR_OK;
  if (pl->deferred >= 0) {
    rc = launch_solve_publish(pl, true);       // the previous tile's solve, then this tile's gate
    if (rc != HSR_OK) return rc;
  } else {
    hipLaunchKernelGGL(gate_kernel, dim3(1), dim3(64), 0, pl->side, pl->sync + 1, pl->published, pl->sync + 2, 1u);
    HSR_LAUNCH_CHECK("gate_kernel");
  }
  int solve_here = 1;
  if (pl->x.host_sum) {
    double* h = pl->host_moments[k];
    rc = hsr::check_hip(hipMemcpyAsync(h, d.moments_dev, nmom * sizeof(double), hipMemcpyDeviceToHost, pl->side), "hsr_pipeline: moments to the host");
    if (rc == HSR_OK) rc = hsr::check_hip(hipLaunchHostFunc(pl->side, host_sum_trampoline, &pl->host_jobs[k]), "hsr_pipeline: host_sum");
    if (rc == HSR_OK) rc = hsr::check_hip(hipMemcpyAsync(d.moments_dev, h, nmom * sizeof(double), hipMemcpyHostToDevice, pl->side), "hsr_pipeline: moments back");
  } else if (pl->x.mode == HSR_SYNC_ALLREDUCE) {
    rc = hsr_allreduce_f64(pl->x.comm, d.moments_dev, nmom, pl->side);
  } else {
    rc = hsr_reduce_f64(pl->x.comm, d.moments_dev, nmom, pl->x.root, pl->side);
    if (rc != HSR_OK) return rc;
    rc = hsr_poly_solve(d.moments_dev, d.nb, d.deg, d.min_count, d.coeffs_dev, pl->side);      // only the root's is kept
    if (rc != HSR_OK) return rc;
    rc = hsr_bcast(pl->x.comm, d.coeffs_dev, (int64_t)d.nb * (d.deg + 1) * (int64_t)sizeof(double), pl->x.root, pl->side);
    solve_here = 0;
  }
  if (rc != HSR_OK) return rc;
  if (pl->x.rehearsal_us > 0) {
    hipLaunchKernelGGL(rehearsal_collective_kernel, dim3(pl->x.rehearsal_blocks > 0 ? pl->x.rehearsal_blocks : 1), dim3(256), 0, pl->side,
                       (int)pl->x.rehearsal_us, pl->sync + 3);
    HSR_LAUNCH_CHECK("rehearsal_collective_kernel");
  }
  pl->deferred = k;
  pl->deferred_solve = solve_here;
  pl->slot[k].exchanged = true;
  return HSR_OK;
}

// ---- T + 2 slots: ONE fit per group of T consecutive tiles (a mosaic held by one GPU) ----------------------------------
// Launch n = K3 of tile n - (T + 1) as the pre-phase | K1+K2 of tile n | slot reduction of tile n - 1 in the tail; the tail of the launch
// that follows a group's LAST tile also adds the group's T per-tile moment sets (the tree of hsr_moments_reduce over T slots) and
// solves.  A tile's K3 therefore rides T + 1 launches later, when its group's polynomial has been ready for at least one launch:
// nothing but one kernel per tile on the caller's stream, no side stream, no events, no CUs kept free.  Buffers of two
// consecutive groups never alias (parity).
static inline size_t group_mom_doubles(const hsr_pipeline* pl) {
  return (size_t)pl->slot[0].p->d.nb * hsr::moment_count(pl->slot[0].p->d.deg);
}
static inline double* group_entry(const hsr_pipeline* pl, int64_t tile) {      // moments of tile `tile` inside its group's array
  const int64_t g = tile / pl->group_T, i = tile % pl->group_T;
  return pl->group_moments + ((size_t)(g & 1) * pl->group_T + (size_t)i) * group_mom_doubles(pl);
}
static inline double* group_total_of(const hsr_pipeline* pl, int64_t tile) { return pl->group_total + (size_t)((tile / pl->group_T) & 1) * group_mom_doubles(pl); }
static inline double* group_coeffs_of(const hsr_pipeline* pl, int64_t tile) {
  return pl->group_coeffs + (size_t)((tile / pl->group_T) & 1) * pl->slot[0].p->d.nb * (pl->slot[0].p->d.deg + 1);
}

// ---- the three fused forms: one submit and one finish path -------------------------------------------------------------
// Launch n = [K3 of tile n - (S - 1) as the pre-phase | K1+K2 of tile n | fit of tile n - 1 in the tail]: tile n - 2 (fused),
// n - 3 (exchange), n - T - 1 (group).  What differs between the forms is in the helpers below, one switch each.

// where the fit of a tile writes its moments, and the coefficients its K3 reads
static inline double* moments_of(hsr_pipeline* pl, int64_t tile) { return pl->kind == kGroup ? group_entry(pl, tile) : slot_of(pl, tile).p->d.moments_dev; }
static inline double* coeffs_of(hsr_pipeline* pl, int64_t tile) { return pl->kind == kGroup ? group_coeffs_of(pl, tile) : slot_of(pl, tile).p->d.coeffs_dev; }

// K3 of `tile` as the pre-phase of a K1 launch
static void job_apply(hsr_pipeline* pl, int64_t tile, const uint8_t* mask, hsr_apply_job* job) {
  const pipe_slot& s = slot_of(pl, tile);
  const hsr_step_desc& d = s.p->d;
  job->x_dev = d.pseudo_dev;
  job->out_dev = d.matched_dev;
  job->coeffs_dev = coeffs_of(pl, tile);
  job->mask_dev = d.apply_mask ? mask : nullptr;
  job->npix = d.npix;
  job->clip = d.clip;
  if (pl->kind == kExchange) {               // the coefficients come from the side stream: wait for the slot's "ready" word
    job->coeffs_ready_dev = pl->sync + 4 + tile % pl->nslots;
    job->coeffs_ready_value = s.seq;
  }
}

// the fit of `tile` in the tail of a K1 launch
static void job_fit(hsr_pipeline* pl, int64_t tile, hsr_apply_job* job) {
  const hsr_step_plan* p = slot_of(pl, tile).p;
  job->fit_partials_dev = p->d.partials_dev;
  job->fit_slots = p->slots;
  job->fit_moments_dev = moments_of(pl, tile);
  job->fit_coeffs_dev = coeffs_of(pl, tile);
  job->fit_min_count = p->d.min_count;
  job->fit_counter_dev = pl->sync;
  job->fit_ticket_base = pl->tickets;
  switch (pl->kind) {
    case kExchange:                          // reduce only, and publish: the solve follows the collective on the side stream
      job->fit_ready_dev = pl->sync + 1;
      break;
    case kGroup: {                           // the tile's entry of its group; behind the group's last tile the group's sum + solve
      const int T = pl->group_T;
      job->fit_group_tiles = T;
      job->fit_group_index = (int32_t)(tile % T);
      job->fit_group_moments_dev = group_entry(pl, tile - tile % T);
      job->fit_group_total_dev = group_total_of(pl, tile);
      break;
    }
  }
}

// the same fit as launches of its own on the caller's stream: for a tile whose follower cannot carry it, or at a drain
static int fit_standalone(hsr_pipeline* pl, int64_t tile, hipStream_t main) {
  pipe_slot& s = slot_of(pl, tile);
  const hsr_step_desc& d = s.p->d;
  int rc = HSR_OK;
  switch (pl->kind) {
    case kFused:
      rc = hsr_moments_reduce_solve(d.partials_dev, s.p->slots, d.nb, d.deg, d.min_count, d.moments_dev, d.coeffs_dev, main);
      break;
    case kExchange:
      rc = hsr_moments_reduce(d.partials_dev, s.p->slots, d.nb, d.deg, d.moments_dev, main);
      if (rc != HSR_OK) return rc;
      hipLaunchKernelGGL(publish_add_kernel, dim3(1), dim3(64), 0, main, pl->sync + 1, (unsigned int)d.nb);
      HSR_LAUNCH_CHECK("publish_add_kernel");
      pl->published += (unsigned int)d.nb;
      break;
    case kGroup: {
      const int T = pl->group_T;
      rc = hsr_moments_reduce(d.partials_dev, s.p->slots, d.nb, d.deg, group_entry(pl, tile), main);
      if (rc == HSR_OK && tile % T == T - 1)
        rc = hsr_moments_reduce_solve(group_entry(pl, tile - (T - 1)), T, d.nb, d.deg, d.min_count, group_total_of(pl, tile),
                                      group_coeffs_of(pl, tile), main);
      break;
    }
  }
  if (rc == HSR_OK) s.fitted = true;
  return rc;
}

static int submit_fused(hsr_pipeline* pl, const void* cube_dev, const float* real_dev, const uint8_t* mask_dev,
                        const uint8_t* prev_mask_dev, hipStream_t main, int32_t* finished_slot, void* k1_begin_event,
                        void* k1_end_event) {
  const int S = pl->nslots;
  const int64_t n = pl->n, old = n - (S - 1), last = n - 1;
  pipe_slot& cur = slot_of(pl, n);
  const bool carry = old >= 0 && slot_of(pl, old).pending;                                  // its K3 rides in this launch
  const bool fit_last = last >= 0 && slot_of(pl, last).pending && !slot_of(pl, last).fitted;
  HSR_REQUIRE(!carry || pl->kind != kExchange || slot_of(pl, old).exchanged, HSR_ERR_INVALID,
              "hsr_pipeline_submit: tile %lld has no exchange enqueued", (long long)old);
  hsr_apply_job job{};
  if (pl->kind == kExchange) job.sync_error_dev = pl->sync + 2;
  if (carry) job_apply(pl, old, prev_mask_dev, &job);
  // Every workgroup of the launch draws ONE ticket and tickets 0 .. nb-1 fit one band each: a launch of fewer workgroups than bands
  // - a tile of fewer than nb 64-pixel groups - cannot carry the fit, which then runs in front of it as launches of its own.  (Found
  // by tools/dbg/stress_fused.py: a 2 x 158 tile with 7 bands kept two stale rows.)
  const int grid = hsr_partial_slots(cur.p->d.npix, &cur.p->d.opts);
  const bool ride = fit_last && grid >= cur.p->d.nb;
  int rc = HSR_OK;
  if (ride) job_fit(pl, last, &job);
  else if (fit_last) rc = fit_standalone(pl, last, main);
  if (rc == HSR_OK) rc = run_k1_timed(cur.p, cube_dev, real_dev, mask_dev, main, (carry || ride) ? &job : nullptr, k1_begin_event, k1_end_event);
  if (rc != HSR_OK) return rc;
  if (ride) {
    // the ticket base advances by the workgroups the launch REALLY had (run_k1 reports them), and that must be the number the
    // "can this launch carry the fit" test above was made with
    HSR_REQUIRE(cur.p->slots == grid, HSR_ERR_INVALID, "hsr_pipeline_submit: the launch used %d workgroups, %d expected", cur.p->slots, grid);
    pl->tickets += (unsigned int)cur.p->slots;
    if (pl->kind == kExchange) pl->published += (unsigned int)cur.p->d.nb;
    slot_of(pl, last).fitted = true;
  }
  // exchange: the moments of tile n - 1 are (or will be, when this launch's tail runs) published - its collective
  if (rc == HSR_OK && fit_last && pl->kind == kExchange) rc = enqueue_exchange(pl, (int)(last % S));
  if (rc != HSR_OK) return rc;
  if (carry) {
    slot_of(pl, old).pending = false;
    if (finished_slot) *finished_slot = (int)(old % S);
  }
  cur.pending = true;
  cur.fitted = cur.exchanged = false;
  cur.seq = (unsigned int)(n + 1);
  pl->n += 1;
  return HSR_OK;
}

// drain: tile i (the oldest unfinished one) outside a K1 launch - its fit enqueued if it is not yet, then K3 as its own launch with
// the tile's coefficients
static int finish_fused(hsr_pipeline* pl, int64_t i, const uint8_t* mask, hipStream_t main) {
  // A group's polynomial needs every reduction of the group: whole groups only, and the open reductions (only the newest tile's can
  // be) go out first.
  HSR_REQUIRE(pl->kind != kGroup || pl->n % pl->group_T == 0, HSR_ERR_INVALID,
              "hsr_pipeline_flush: %lld tiles submitted, not a whole number of groups of %d - the last group has no fit yet", (long long)pl->n, pl->group_T);
  int rc = HSR_OK;
  if (pl->kind == kFused && i + 1 < pl->n && slot_of(pl, i).fitted && slot_of(pl, i + 1).pending && !slot_of(pl, i + 1).fitted) {
    // Two tiles left: this one's K3 and the newest one's fit are the two ends of a carrying launch - one kernel instead of K3 here and
    // reduce + solve in front of the last K3.  Same rule as `ride` in submit_fused: at least nb workgroups, else the launches below.
    pipe_slot& s = slot_of(pl, i);
    const hsr_step_desc& d = s.p->d;
    const int grid = hsr_partial_slots(d.npix, &d.opts);
    if (grid >= d.nb) {
      hsr_apply_job job{};
      job_apply(pl, i, mask, &job);
      job_fit(pl, i + 1, &job);
      job.fit_counter_dev = pl->sync + kSyncDrainTickets;
      job.fit_ticket_base = pl->drain_tickets;
      rc = run_drain(job, d, grid, main);
      if (rc != HSR_OK) return rc;
      pl->drain_tickets += (unsigned int)grid;
      slot_of(pl, i + 1).fitted = true;
      s.pending = false;
      return HSR_OK;
    }
  }
  for (int64_t k = i; k < (pl->kind == kGroup ? pl->n : i + 1) && rc == HSR_OK; ++k)
    if (slot_of(pl, k).pending && !slot_of(pl, k).fitted) rc = fit_standalone(pl, k, main);
  pipe_slot& s = slot_of(pl, i);
  if (pl->kind == kExchange) {
    if (rc == HSR_OK && !s.exchanged) rc = enqueue_exchange(pl, (int)(i % pl->nslots));
    if (rc == HSR_OK && pl->deferred >= 0) rc = launch_solve_publish(pl, false);     // (this tile's, or a later one's: at most one is deferred)
    // (an EVENT here, not a polling gate: this is a drain, a bubble costs nothing - and a wave spinning on the caller's stream would
    // deadlock, until its time limit, against side-stream work queued behind it if the runtime serves both streams from one
    // hardware queue.  Everything the side stream still holds in front of the record is released by launches that are already
    // enqueued on the caller's stream.)
    if (rc == HSR_OK) rc = hsr::check_hip(hipEventRecord(s.ev_fit, pl->side), "hsr_pipeline: record fit");
    if (rc == HSR_OK) rc = hsr::check_hip(hipStreamWaitEvent(main, s.ev_fit, 0), "hsr_pipeline: wait for the fit");
  }
  if (rc != HSR_OK) return rc;
  rc = run_apply(s.p, coeffs_of(pl, i), mask, main);
  s.pending = false;
  return rc;
}

// ---- two slots: the fit on the side stream, K3 as its own launch ---------------------------------------------------------
static int finish_two_slot(pipe_slot& s, const uint8_t* mask, hipStream_t main) {
  int rc = hsr::check_hip(hipStreamWaitEvent(main, s.ev_fit, 0), "hsr_pipeline: wait for the fit");
  if (rc != HSR_OK) return rc;
  rc = run_apply(s.p, s.p->d.coeffs_dev, mask, main);
  s.pending = false;
  return rc;
}

static int submit_two_slot(hsr_pipeline* pl, const void* cube_dev, const float* real_dev, const uint8_t* mask_dev,
                           const uint8_t* prev_mask_dev, hipStream_t main, int32_t* finished_slot, void* k1_begin_event,
                           void* k1_end_event) {
  const int cur = (int)(pl->n % 2);
  pipe_slot &s = pl->slot[cur], &prev = pl->slot[cur ^ 1];
  int rc = HSR_OK;
  rc = run_k1_timed(s.p, cube_dev, real_dev, mask_dev, main, nullptr, k1_begin_event, k1_end_event);
  if (rc != HSR_OK) return rc;
  if (prev.pending) {
    rc = finish_two_slot(prev, prev_mask_dev, main);
    if (rc != HSR_OK) return rc;
    if (finished_slot) *finished_slot = cur ^ 1;
  }
  rc = hsr::check_hip(hipEventRecord(s.ev_k1, main), "hsr_pipeline: record K1");
  if (rc == HSR_OK) rc = hsr::check_hip(hipStreamWaitEvent(pl->side, s.ev_k1, 0), "hsr_pipeline: side stream wait");
  if (rc == HSR_OK && !pl->exchange) {
    const hsr_step_desc& d = s.p->d;
    rc = hsr_moments_reduce_solve(d.partials_dev, s.p->slots, d.nb, d.deg, d.min_count, d.moments_dev, d.coeffs_dev, pl->side);
    if (rc == HSR_OK) rc = hsr::check_hip(hipEventRecord(s.ev_fit, pl->side), "hsr_pipeline: record fit");
  }
  if (rc != HSR_OK) return rc;
  s.pending = true;
  pl->n += 1;
  return HSR_OK;
}

// Starts tile i in slot i % S and finishes tile i-1 (two slots), i-2 (fused), i-3 (fused with exchange) or i-T-1 (group): its K3.
// *finished_slot = slot of the finished tile, or -1.  prev_mask_dev: the mask of the tile being finished (only read when the
// plan applies the mask in K3).
// Two slots, exchange = 0: the fit (slot reduction + solve) is enqueued on the side stream here.  With exchange = 1 the side stream
// has been made to wait for K1(i) when this returns; the caller enqueues reduce -> collective -> solve on it and then calls
// hsr_pipeline_fit_done.
extern "C" int hsr_pipeline_submit(hsr_pipeline* pl, const void* cube_dev, const float* real_dev, const uint8_t* mask_dev,
                                   const uint8_t* prev_mask_dev, hsr_stream_t main_stream, int32_t* finished_slot,
                                   void* k1_begin_event, void* k1_end_event) {
  HSR_REQUIRE(pl && cube_dev && real_dev, HSR_ERR_INVALID, "hsr_pipeline_submit: NULL argument");
  const int cur = (int)(pl->n % pl->nslots);
  HSR_REQUIRE(!pl->slot[cur].pending, HSR_ERR_INVALID, "hsr_pipeline_submit: slot %d still holds an unfinished tile", cur);
  if (finished_slot) *finished_slot = -1;
  hipStream_t main = (hipStream_t)main_stream;
  if (pl->kind == kTwoSlot) return submit_two_slot(pl, cube_dev, real_dev, mask_dev, prev_mask_dev, main, finished_slot, k1_begin_event, k1_end_event);
  return submit_fused(pl, cube_dev, real_dev, mask_dev, prev_mask_dev, main, finished_slot, k1_begin_event, k1_end_event);
}

// two slots, exchange = 1: the caller has enqueued the fit of the slot submitted last on the side stream.
extern "C" int hsr_pipeline_fit_done(hsr_pipeline* pl) {
  HSR_REQUIRE(pl && pl->n > 0 && pl->kind == kTwoSlot, HSR_ERR_INVALID, "hsr_pipeline_fit_done: nothing submitted, or not a two-slot pipeline");
  return hsr::check_hip(hipEventRecord(slot_of(pl, pl->n - 1).ev_fit, pl->side), "hsr_pipeline: record fit");
}

// K3 of the OLDEST tile left in the pipeline; *finished_slot = its slot or -1.
extern "C" int hsr_pipeline_flush(hsr_pipeline* pl, const uint8_t* mask_dev, hsr_stream_t main_stream, int32_t* finished_slot) {
  HSR_REQUIRE(pl, HSR_ERR_INVALID, "hsr_pipeline_flush: NULL pipeline");
  if (finished_slot) *finished_slot = -1;
  const int S = pl->nslots;
  for (int64_t i = pl->n >= S - 1 ? pl->n - (S - 1) : 0; i < pl->n; ++i) {
    pipe_slot& s = slot_of(pl, i);
    if (!s.pending) continue;
    const int rc = pl->kind == kTwoSlot ? finish_two_slot(s, mask_dev, (hipStream_t)main_stream)
                                        : finish_fused(pl, i, mask_dev, (hipStream_t)main_stream);
    if (rc == HSR_OK && finished_slot) *finished_slot = (int)(i % S);
    return rc;
  }
  return HSR_OK;
}

extern "C" int64_t hsr_pipeline_count(const hsr_pipeline* pl) { return pl ? pl->n : -1; }

extern "C" int hsr_pipeline_status(hsr_pipeline* pl, hsr_stream_t main_stream, uint32_t* sync_error_out) {
  HSR_REQUIRE(pl && sync_error_out, HSR_ERR_INVALID, "hsr_pipeline_status: NULL argument");
  *sync_error_out = 0;
  int rc = hsr::check_hip(hipStreamSynchronize((hipStream_t)main_stream), "hsr_pipeline_status: caller's stream");
  if (rc == HSR_OK) rc = hsr::check_hip(hipStreamSynchronize(pl->side), "hsr_pipeline_status: side stream");
  if (rc != HSR_OK || !pl->sync) return rc;
  unsigned int code = 0;
  rc = hsr::check_hip(hipMemcpy(&code, pl->sync + 2, sizeof code, hipMemcpyDeviceToHost), "hsr_pipeline_status: read the error word");
  *sync_error_out = code | (pl->host_error ? 16u : 0u);
  return rc;
}
