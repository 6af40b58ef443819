// ks_hip.hip — MI355X (gfx950) semantic TSDF integrator: HIP kernels + the C ABI of include/ks_hip.h.
//
// Replaces, behind the reference's plugin surface, the CPU hot path
//   kimera::FastSemanticTsdfIntegrator::integratePointCloud    [K:src/semantic_tsdf_integrator_fast.cpp:57-199]
//   kimera::MergedSemanticTsdfIntegrator::integratePointCloud  [K:src/semantic_tsdf_integrator_merged.cpp:65-329]
//   kimera::SemanticIntegratorBase::updateSemanticVoxel         [K:src/semantic_integrator_base.cpp:136-194, 283-380]
// ([K:...] = path under /root/reference/kimera_semantics/).
//
// Per frame (no CPU fallback exists):
//   stage A  points  : one lane per point — validity, T_G_C * p, start-voxel / end-voxel key  (k_points_*)
//            sort    : radix sort of point keys (start-voxel dedup slots | end-voxel bundles)   (ks_radix_sort.h)
//            rays    : exact sequential-equivalent dedup (fast) or per-bundle merge (merged)   (k_dedup / k_bundles)
//   stage B  early-out: (fast) ordered phases of k_test decide how far every ray gets (and enter its marks)        (ks_k_march.h)
//            emit    : scan of the per-position update counts, then every ray writes its (voxel, position)
//                      pairs at its own offset, allocating tiles in the spatial hash              (k_scan_local, k_emit_lane)
//            publish : pair / ray / tile counts -> pinned host memory                           (k_publish)
//   stage T  sort    : stable radix sort of the pairs on the voxel bits => every voxel's updates contiguous,
//                      in reference order (the pair list is emitted in integration order)
//            apply   : 8 lanes per voxel run — sequential TSDF + log-likelihood update, one
//                      128-byte record read and written once; runs of >= 32 updates get a workgroup each
//                      on a second stream                                                        (k_find_long, k_apply, k_apply_long)
// Kernels live in ks_k_rays.h / ks_k_march.h / ks_k_apply.h / ks_k_io.h (types: ks_types.h); this
// file is the host side: context, frame slots, the three-stream frame pipeline, the C ABI.
// Ordering contract: per voxel, updates are applied in exactly the order the reference's
// single-threaded integrator would apply them, which makes labels bit-exact.
//
// Data layout in HBM: 8x8x8-voxel tiles of 128-byte voxel records (dist | weight | colour | label
// | 21 class priors), addressed through an open-addressing hash table keyed by the packed tile index.

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cstring>
#include <string.h>

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <iterator>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ks_hip.h"
#include "ks_device_math.h"
#include "ks_owned.h"
#include "ks_radix_sort.h"

using namespace ksd;

#include "ks_types.h"
#include "ks_k_bundle_order.h"
#include "ks_k_rays.h"
#include "ks_k_march.h"
#include "ks_k_exact.h"
#include "ks_k_apply.h"
#include "ks_k_apply_xl.h"
#include "ks_k_shard.h"
#include "ks_k_shard_merged.h"
#include "ks_k_io.h"
#include "ks_k_mesh.h"
#include "ks_k_mesh_index.h"
#include "ks_k_esdf.h"
#include "ks_k_esdf_read.h"
#include "ks_k_render.h"
#include "ks_k_align.h"
#include "ks_k_objects.h"
#include "ks_k_nav.h"
#include "ks_k_frontier.h"
#include "ks_k_rooms.h"
#include "ks_k_view_gain.h"
#include "ks_k_path.h"
#include "ks_k_remove.h"
#include "ks_k_fuse.h"

using namespace ksk;

namespace {

std::string g_create_error;

// Every diagnostic / A-B switch of the library sits behind ONE gate: without KS_DEBUG=1 in the environment none of them is
// read.  None changes a map (equivalent launch strategies, test sizes of buffers, traces); tests and tools that use one
// set KS_DEBUG=1 beside it.
const char* dbg_env(const char* name) {
  const char* g = getenv("KS_DEBUG");   // (read per ks_create: a test process sets and clears it between contexts)
  return (g && g[0] == '1') ? getenv(name) : nullptr;
}

}  // namespace

// ==========================================================================================
// Host side of the C ABI
// ==========================================================================================
// Everything a later stage reads from an earlier one lives in a FrameSlot.  With
// ks_config.pipeline_frames the stages of a frame run on separate streams,
//   A  points -> sort -> dedup / bundles                  (stream)
//   B  early-out phases, scan, emission, snapshot          (one of the march streams: frame % n_march)
//   T  init tiles -> sort pairs -> find_long -> apply       (stream_tail; k_apply_long beside it on stream_long, k_apply_xlong
//      on stream_xlong — or both behind it on stream_tail where the process has fewer hardware queues than the context
//      has chains: stream_plan), enqueued by a helper thread 1..8 calls later
// so that A, B and T of neighbouring frames execute concurrently: B is a chain of small dependent launches
// (replayed as a graph captured once per slot), the sorts are bound by dependent-launch latency, the voxel
// update by memory latency, and neither A nor B touches voxel data.  The host's one wait per frame (for the
// snapshot that sizes T) never idles the GPU.  Twelve slots rotate (24 above a lag of 8); stage A of a frame waits for the tail (and
// the long runs) that last used its slot.
constexpr int kMaxLag = 16;          // largest ks_config.pipeline_frames
constexpr int kSlots = kMaxLag + 8;  // frame slots at most; a context uses ks_ctx::n_slots of them: 12 up to a lag of 8 (three batches
                                     // of four), 24 above (three batches of eight) — the tail may lag up to kMaxLag calls
constexpr int kMarchStreams = 8;
constexpr int kObsTables = 16;       // early-out tables at most; a context uses n_obs = batch x march streams of them: one per frame whose stage B
                                     // can be in flight (8 today: two batches of four, or one of eight)
struct HostSnap {
  Counters c;
  uint32_t n_tiles;
  uint32_t pad[7];
};
struct FrameSlot {
  int index = 0;
  DevBuf<RayDesc> d_rays;
  DevBuf<float> d_deltas;           // merged: label histograms of mixed bundles
  DevBuf<uint64_t> d_pairs;         // (voxel, ray) pairs in integration order, written by k_emit
  DevBuf<uint32_t> d_cnt;           // updates per integration position (merged: 2 n entries)
  DevBuf<uint32_t> d_lp;            // exclusive prefix of d_cnt inside blocks of kScanBlock
  DevBuf<unsigned long long> d_bt;  // block totals of that scan
  DevBuf<uint8_t> d_live;           // fast: position holds a ray that survived start-voxel dedup
  DevBuf<uint32_t> d_seed_gen, d_seed_items, d_seed_n;   // early-out: the seed's work list (k_seed_list -> k_test)
  bool wide = false;                // stage B uses a whole wavefront per ray (long rays)
  DevBuf<FrameParams> d_F;          // the frame's parameters in device memory (stage B reads them from there)
  DevBuf<uint64_t> d_gkeys, d_rkeys;  // anti-grazing: this frame's sorted end-voxel keys / key per bundle
  // stage B of the batch that STARTS on this slot as captured graphs, valid for a (point count, buffers, batch size) key.
  // Exact early-out, event-driven fix point (ks_k_exact.h): THREE graphs (seed + marks + bulk rounds | finisher + commit |
  // scan + emission) with the wait for the previous frame's commit between the first two; otherwise g1 alone.
  // Two sets: [0] full batches, [1] partial ones (a flush ends a batch early: a stream that is flushed every K frames, K no
  // multiple of the batch, would otherwise re-capture on every change of the size).
  struct GraphSet {   // owns its graphs
    hipGraphExec_t g1 = nullptr, g2 = nullptr, g3 = nullptr;
    uint64_t key = 0;
    GraphSet() = default;
    GraphSet(const GraphSet&) = delete;
    GraphSet& operator=(const GraphSet&) = delete;
    ~GraphSet() { reset(); }
    void reset() {
      for (hipGraphExec_t* g : {&g1, &g2, &g3}) {
        if (*g) (void)hipGraphExecDestroy(*g);
        *g = nullptr;
      }
      key = 0;
    }
  } b_graphs[2];
  // exact early-out, event-driven fix point (ks_k_exact.h): the slot's marks, per-slot table, X marks, lists
  DevBuf<uint64_t> d_eo_keys[2];
  DevBuf<uint32_t> d_eo_vals[2];
  size_t eo_cap_marks = 0;          // of the marks' group: keys, values, sort workspace, hit bytes, hseq, where, the two bitmaps
  DevBuf<uint4> d_eo_tab;
  DevBuf<unsigned long long> d_eo_xnode;   // [2 x X marks]
  DevBuf<uint32_t> d_eo_cnt_b, d_eo_ux, d_eo_dirty, d_eo_list[2], d_eo_chg, d_eo_consulted, d_eo_lp;
  DevBuf<unsigned long long> d_eo_bt;
  DevBuf<EoCtl> d_eo_ctl;
  DevBuf<uint32_t> d_eo_sort_ws;
  DevBuf<uint32_t> d_eo_hseq, d_eo_where;   // per seed mark in emission order: voxel hash | index in M
  DevBuf<uint4> d_eo_rinfo, d_eo_ckpt;      // per position: {u0, um, length, checkpoint step} | caster state there
  DevBuf<uint8_t> d_eo_hitb;                // first iteration: per mark in emission order, the visit is a hit
  DevBuf<unsigned long long> d_eo_bits_a, d_eo_bits_b;   // per mark of M: it counts under the current / next lengths
  DevBuf<unsigned long long> d_eo_btp;      // ... exclusive prefix of the scan's block totals
  Event eo_committed;               // the frame's marks have entered the shared table
  Counters* d_counters = nullptr;   // a VIEW: inside ks_ctx::d_state
  DevBuf<uint32_t> d_ray_list;      // rays to march (written by stage A, read by B)
  PinnedBuf<HostSnap> h_snap;       // pinned + device-visible: written by k_publish at the end of B
  Event a_done;                     // stage A complete
  Event ready;                      // snapshot has landed
  Event tail_done;                  // the tail has consumed this slot's buffers
  Event fork, join;                 // tail: pairs sorted and long runs listed | long runs applied
  Event join_x;                     // the runs of more than kXLongRun updates applied (stream_xlong)
  Event found;                      // the long runs listed on the long-run stream (k_find_long beside k_apply_runs)
  bool tail_recorded = false;
  bool join_recorded = false;
  bool b_launched = false;    // stage B of the frame has been enqueued (with its batch)
  // the batch the frame's stage B went out with (launch_batch): its index in it, the batch's size and slots in frame order
  int batch_index = 0, batch_nb = 1;
  FrameSlot* batch_slots[kBatchMax] = {};
  bool tail_batched = false;  // the frame's updates were applied with its whole batch's, at the tail of the batch's first frame (tail_batch)
  uint32_t tb_blocks = 0;     // ... and the tiles that tail made valid on this frame's account (ks_frame_stats::n_blocks_allocated)
  size_t steps_max = 0;       // longest possible ray of the frame, in voxels
  uint64_t frame_no = 0;      // the frame the slot holds
  FrameParams F{};
  size_t n = 0;
  int prof_set = -1;
  bool pending = false;
  const Counters& counters() const { return h_snap->c; }
  uint32_t n_tiles() const { return h_snap->n_tiles; }
};

// HIP-event sets for ks_profile: recorded in stream order, resolved lazily (before reuse or in
// ks_profile_get) so that profiling never adds a host wait to a frame.
constexpr int kProfSets = 32;   // 2 x the largest lag (kMaxLag = 16): a set is reused 32 frames later, long after its frame's tail
constexpr int kStageEvents = KS_STAGE_COUNT + 3;  // 0..3 stage A | 4,5 march begin/end | 6 tail begin, 7..10
struct ProfSet {
  Event ev[kStageEvents];
  Event k0, k1;  // begin/end of the k_apply dispatch itself
  bool used = false, complete = false, stages = false, apply = false, applied = false;
  uint64_t n_pairs = 0, n_points = 0;
  uint64_t n_applied = 0;   // updates the timed k_apply launch applied: the frame's, or its whole batch's (tail_batch)
};

// ---- the stream plan: which chain of a frame runs on which stream -------------------------------------------------------
// The runtime spreads a process's streams over its hardware queues (GPU_MAX_HW_QUEUES of them: four unless the host says
// otherwise), and kernels of streams that share a queue run one after the other.  A context that asks for more streams than
// there are queues leaves it to the runtime which two of its chains serialise — a stage-B chain of 2 ms with the 9 us of the
// runs of more than kXLongRun updates, say, whose fork and join then wait in line behind it.  So the two light
// side chains of stage T give up their streams first: they run ON the tail stream, in order behind k_apply (the same
// hipStream_t: an alias, a view like every named handle of ks_ctx), until the context fits the budget or nothing light is left.
// Stage A, the march streams and stage T never fold.
struct StreamPlanIn {
  bool uses_early_out = false;       // `fast` whose consecutive-collision limit can fire: stage B is a chain of its own
  bool exact_early_out = false;      // ... in the reference's serial order (the default mode)
  bool frames_independent = true;    // a frame's early-out marks are never seen by the next frame
  int pipeline_frames = 0;           // as in effect (ks_create may have reduced ks_config's)
  int batch = 1;                     // frames per stage-B launch sequence
  bool xlong = true;                 // the runs of more than kXLongRun updates have a kernel of their own (KS_XLONG)
  int budget = 4;                    // hardware queues of the process
};
struct StreamPlan {
  int budget = 4;
  int n_march = 1;
  bool march_own = false;            // stage B on streams of its own (else: stage A's)
  bool tail_own = false;             // stage T on a stream of its own (else: stage A's)
  bool long_own = true;              // k_apply_long beside k_apply (else: on the tail stream, behind it)
  bool xlong_own = true;             // k_apply_xlong beside both (else: on the tail stream); false without xlong
  int distinct = 1;                  // streams the context creates
};
inline StreamPlan stream_plan(const StreamPlanIn& in) {
  StreamPlan p;
  p.budget = in.budget;
  if (in.pipeline_frames) {
    // (shared early-out table: stage B of consecutive frames stays in order on one stream)
    p.n_march = (!in.frames_independent || in.batch > 1) ? 1 : std::min(kMarchStreams, std::max(4, in.pipeline_frames));
    // (exact early-out: a frame's stage B is a chain of ~75 small launches, ~1.5 ms long, and the hardware runs two or three
    // such chains side by side at best — measured: 8 streams lose to 4.  With pipeline_frames = 8 the chain is shared by
    // the four frames of a batch, and two batches alternate over two streams.)
    if (in.exact_early_out && p.n_march > 4) p.n_march = 4;
    if (in.exact_early_out && in.batch > 1) p.n_march = 2;
    // without an early-out stage B is short (scan + emission): it follows stage A on the same stream
    if (!in.uses_early_out) p.n_march = 1;
    p.march_own = in.uses_early_out;
    p.tail_own = true;
  }
  p.long_own = true;
  p.xlong_own = in.xlong;
  auto count = [&p] { return 1 + (p.march_own ? p.n_march : 0) + (p.tail_own ? 1 : 0) + (p.long_own ? 1 : 0) + (p.xlong_own ? 1 : 0); };
  // (from eight queues on — what INTEGRATION.md 4.2 recommends and every layout was measured under — nothing folds)
  if (p.budget < 8 && count() > p.budget) p.xlong_own = false;
  if (p.budget < 8 && count() > p.budget) p.long_own = false;
  p.distinct = count();
  return p;
}
// Hardware queues of this process: what the runtime will read from GPU_MAX_HW_QUEUES (only read here, never set: the library
// changes nothing in its host's environment), four — the runtime's default — when it is unset or no number.
// KS_DEBUG=1 KS_HW_QUEUES=<n> (tests / A-B) overrides the budget of the plan; the runtime's queues stay what they are.
inline int hw_queue_budget() {
  auto number = [](const char* s, int* out) {
    if (!s) return false;
    char* end = nullptr;
    const long v = strtol(s, &end, 10);
    if (end == s) return false;
    *out = (int)std::min<long>(32, std::max<long>(1, v));
    return true;
  };
  int b = 4;
  number(getenv("GPU_MAX_HW_QUEUES"), &b);
  number(dbg_env("KS_HW_QUEUES"), &b);
  return b;
}

// MEMBER ORDER IS TEARDOWN ORDER, reversed: the stream owners come first, so `delete c` frees every buffer, pinned block,
// event and graph before it destroys the streams whose work referred to them (ks_destroy has synchronised them all).
struct ks_ctx {
  Stream streams[kMarchStreams + 4];   // every stream of the context, in creation order; the named handles below are views
  int n_streams = 0;
  ks_config cfg{};
  std::string err;
  hipStream_t stream = nullptr;        // stage A (and everything else)
  // stage B; == stream unless pipelined.  Pipelined, consecutive frames march on kMarchStreams streams in
  // turn (stage B of frame i+1 does not depend on stage B of frame i: tile allocation is atomic, and the
  // early-out set of a frame is private to it when every frame bumps the set offset — then each stream
  // has its own table)
  hipStream_t stream_march_[kMarchStreams] = {};
  int n_march = 1;
  int batch = 1;                        // frames whose stage B is launched together (ks_k_march.h: BatchView)
  std::vector<FrameSlot*> batch_slots;  // frames whose stage A is enqueued and whose stage B waits for the batch to fill
  hipStream_t prof_march_stream = nullptr;  // march stream of the frame being enqueued (stage events)
  hipStream_t stream_tail = nullptr;   // stage T; == stream unless pipelined
  hipStream_t stream_long = nullptr;   // the long-run voxel update, beside k_apply (== stream_tail where the plan folds it)
  hipStream_t stream_xlong = nullptr;  // the runs of more than kXLongRun updates, beside both (k_apply_xlong; == stream_tail where folded)
  StreamPlan plan;                     // what ks_create made the streams from (ks_stream_plan)
  bool xlong = true;
  float voxel_size_inv = 0.f, log_match = 0.f, log_non_match = 0.f;
  int vps_shift = 1;  // log2(vps / 8)

  TileTable table{};                   // views of table_ent, table_slot_keys and (n_tiles) d_state
  Pool pool{};                         // views of pool_vox, pool_updated, pool_dirty
  DevBuf<TileEntry> table_ent;
  DevBuf<uint64_t> table_slot_keys;
  DevBuf<uint4> pool_vox;
  DevBuf<uint8_t> pool_updated, pool_dirty;
  DevBuf<uint64_t> d_start_set;
  DevBuf<uint64_t> d_observed_[kObsTables];
  int n_obs = 1;
  uint64_t start_offset = 0, observed_offset = 0;
  int64_t reset_counter = 0;
  uint32_t obs_tag = 0, obs_tag_lo = 1;  // frame tag of the observed set's entries (ks_k_march.h)
  DevBuf<Counters> d_retry_counters;     // scratch of the pair-buffer overflow retry
  std::atomic<size_t> pairs_hint{0};     // largest pair count of a frame so far (written by the thread that runs the tails, read by the caller's)
  bool uses_early_out = false;           // fast integrator whose consecutive-collision limit can fire
  // the seed's launch shape for cap_points (seed_launch_shape; ensure_points): per phase its generations, its part of the
  // slots' item lists and the wavefronts launched per frame — on the host for stage B's grids, on the device for k_seed_list
  std::vector<SeedPhase> seed_phases;
  DevBuf<SeedPhase> d_seed_phases;
  size_t seed_cap_items = 0;             // KS_DEBUG=1 KS_SEED_CAP_ITEMS=<n>: no phase's launch covers more items (tests: the overflow guard)
  // Pipelined contexts enqueue the tail of frame i-lag on a helper thread while the calling thread enqueues
  // stages A and B of frame i (the host, not the GPU, bounds small frames: ~25 launches of ~8 us each per
  // frame).  The call still returns only after both are done, so what a call delivers does not change.
  std::thread tail_thread;
  std::mutex tail_mu;
  std::mutex capture_mu;           // a stream capture (caller) never overlaps a tail being enqueued (helper): the tail may
                                   // allocate, free or synchronise, which a capture in progress on another thread does not survive reliably
  std::condition_variable tail_cv;
  FrameSlot* tail_job = nullptr;   // posted by the caller, taken by the helper
  bool tail_busy = false, tail_quit = false;
  int tail_rc = KS_OK;
  bool use_tail_thread = false;
  bool use_graphs = true;                // stage B replayed as a hipGraph (a capture failure: plain launches)
  bool test_overlap = true;              // k_test casts a long ray's next 64 voxels while the shared-set entries of the current 64 are in flight (KS_TEST_OVERLAP=0: one after the other, as measured until round 3)
  std::atomic<uint64_t> buffers_epoch{1};  // bumped whenever a buffer a captured graph points at is re-allocated
  DevBuf<uint8_t> d_color_lut;      // 16 MiB rgb -> label
  DevBuf<uint32_t> d_label_lut;     // 256 label -> rgba
  uint32_t tiles_initialised = 0;

  // per-frame buffers
  size_t cap_points = 0;
  DevBuf<float> d_xyz;
  DevBuf<uint8_t> d_rgba;
  DevBuf<uint8_t> d_labels;
  DevBuf<uint32_t> d_hash;
  DevBuf<uint32_t> d_skeys32, d_skeys32b;
  DevBuf<float4> d_gpw;
  DevBuf<uint64_t> d_ray_keys;
  DevBuf<uint2> d_glc;
  // stage T's shared buffers exist twice (frame parity): the long runs of frame f may still be applied from
  // set f & 1 while frame f+1 sorts its pairs and lists its long runs into the other set (deferred join)
  DevBuf<unsigned long long> d_long_list_[2];
  DevBuf<uint32_t> d_blong;
  // merged, reference bundle order: the epochs of the rehash recurrence are launched for this many bundles (the counts of the
  // frames before, with a margin; ~0: as many as the frame has points) — k_bo_rest completes a frame that has more
  std::atomic<uint32_t> bo_hint{~0u};
  bool bo_hint_fixed = false;
  DevBuf<uint64_t> d_key_overflow;      // merged, compact grouping keys: the table of the end voxels outside the key window (k_points_merged)
  uint32_t key_overflow_mask = 0;
  uint32_t key_bits = 0;                // bits per axis of the key window; 0: the 64-bit keys are sorted (FrameParams::key_bits)
  DevBuf<uint64_t> d_pkeys, d_pkeys2;
  DevBuf<uint32_t> d_pvals, d_pvals2;
  DevBuf<uint32_t> d_order;
  DevBuf<uint32_t> d_inv_order;
  DevBuf<uint32_t> d_okeys, d_okeys2, d_ovals;
  size_t cap_pairs = 0;
  DevBuf<uint64_t> d_pairs2_[2];
  // the tail of a whole batch in one pass (tail_batch): the batch's pair lists one behind the other (the sort's input) and its
  // frame table, by parity like the sets above
  DevBuf<uint64_t> d_pairs_cat_[2];
  DevBuf<TailFrame> d_tail_frames_[2];
  size_t cap_cat = 0;
  int last_par = -1;                     // parity set of the last update enqueued
  bool tail_batch_on = true;             // KS_DEBUG=1 KS_TAIL_BATCH=0 (tests / A-B): every frame's tail on its own
  uint64_t tb_stats[4] = {0, 0, 0, 0};   // batches applied in one pass | frames in them | batches that went frame by frame | pairs of the first (ks_tail_batch_stats)
  hipEvent_t pending_join = nullptr;     // (a view: some slot's join) recorded on stream_long; the next k_apply / k_apply_long wait for it
  ksrs::Workspace sort_ws, sort_ws_tail;
  // fast, early-out in the reference's serial order (ks_k_exact.h): marks (two sets for the sort), slot ranges,
  // the reference's table content, the scan of the visited lengths, the iteration's counters
  bool exact_early_out = false;
  DevBuf<uint64_t> d_eo_keys[2];
  DevBuf<uint32_t> d_eo_vals[2];
  size_t cap_marks = 0;
  DevBuf<uint2> d_eo_range;
  DevBuf<uint64_t> d_eo_plain;
  DevBuf<uint32_t> d_eo_lp;
  DevBuf<unsigned long long> d_eo_bt;
  DevBuf<EoState> d_eo_state;
  PinnedBuf<EoState> h_eo_state;
  uint64_t eo_iterations = 0, eo_frames = 0;  // statistics (ks_exact_early_out_stats)
  // ... event-driven (the default; KS_EXACT_HOST_LOOP=1: every frame through the host-driven loop above)
  bool eo_device = false;
  int eo_bulk_rounds = 6;                // rounds enqueued as launches before the one-workgroup finisher takes over
  static constexpr int eo_sweeps = 12;   // long rays: sweeps enqueued at a time (they end themselves once one changes nothing); the host looks
                                         // at the count once per such chunk (launch_batch) and enqueues more while rays still change
  int eo_sweep_chunks = 16;              // ... at most this many chunks, then the host-driven loop takes the frame
  std::atomic<int> eo_want_bulk{0};      // ... as a frame whose finisher was handed too long a list asks for (applied by the caller's thread between frames)
  DevBuf<uint32_t> d_eo_committed;       // frames [0, *d_eo_committed) of the exact path have entered d_eo_plain
  uint32_t eo_frame_no = 0;              // frames launched through the exact path
  hipEvent_t eo_last_commit = nullptr;   // (a view: some slot's eo_committed) commit event of the previous frame (nullptr: nothing to wait for)
  std::atomic<size_t> eo_want_marks{0}, eo_want_x{0};   // capacities a failed frame asked for (grown by the caller's thread between frames)
  size_t eo_cap_marks = 0, eo_cap_x = 0; // per-slot capacities in use
  std::atomic<uint64_t> eo_fallbacks{0}; // frames that fell back to the host-driven loop (counted by the thread that runs the tails)
  uint64_t eo_fallbacks_seen = 0;        // ... as of the caller's last look
  std::atomic<int> eo_hopeless{0};       // consecutive frames the device loop gave up on for reasons growing a buffer does not cure
  bool eo_device_off = false;            // ... three of them: the context stays with the host-driven loop (one frame at a time)
  // merged in the reference's bundle order (ks_k_bundle_order.h): scratch of the rank computation, one slab
  bool use_bundle_rank = false;
  BoCtx bo{};                            // views into d_bo_slab
  BoSchedule bo_sched{};
  DevBuf<uint8_t> d_bo_slab;
  int bo_epochs = 0;                     // epochs launched per frame (those a cloud of cap_points could reach)
  // ks_reduce: grow-only exchange scratch (send / receive keys and raw tile records, per-owner counts)
  DevBuf<int32_t> d_rx_counts;           // [(world + 3) x world]
  DevBuf<uint64_t> d_tx_keys, d_rx_keys;
  DevBuf<uint32_t> d_tx_slots;
  DevBuf<uint8_t> d_tx_payload, d_rx_payload;
  size_t cap_tx = 0, cap_rx = 0;
  // scratch of the multi-GPU exchange entry points (slots / group offsets + order / distinct keys)
  DevBuf<uint32_t> d_xchg_u32;           // [2 x d_xchg_u64.size() + 2]
  DevBuf<uint64_t> d_xchg_u64;
  // Device words: Counters of slot k at 64 * k, the persistent tile count at 64 * kSlots.
  DevBuf<uint8_t> d_state;
  FrameSlot slot[kSlots];
  int n_slots = 1;   // slots in use: 1 (unpipelined), 12 or 24 (ks_create)
  uint64_t frame_no = 0;
  ks_frame_stats owed{};  // statistics of frames completed but not yet handed to the caller (summed)
  DevBuf<int32_t> d_block_idx;
  DevBuf<uint8_t> d_tsdf_out, d_sem_out;
  DevBuf<uint8_t> d_vox_out;        // staging of ks_download_updated_voxels
  size_t cap_out_blocks = 0;        // of the staging group: d_tsdf_out, d_sem_out, d_block_idx

  DevBuf<uint32_t> d_depth_blocks;
  DevBuf<uint8_t> d_img_depth;
  DevBuf<uint8_t> d_img_aux;

  int profiling = 0;  // 0 off, 1 all stages + every k_apply, 2 every 4th k_apply only
  // the voxel update of the short runs: k_apply_runs (a lane per run, runs bucketed by length: ks_k_apply.h) from this many
  // pairs per frame on, k_apply (eight lanes per voxel) below — the same records either way
  unsigned long long apply_runs_min_pairs = 1ull << 20;
  // the runs of more than kXLongRun updates through integer sums per chunk (ks_k_apply_xl.h); one set of buffers: all of it
  // runs in order on stream_xlong
  bool xl_parallel = true;
  unsigned long long xl_min_pairs = 1ull << 23;   // (below: the five launches of the path cost a 640x480 frame more than its handful of such runs through k_apply_xlong)
  DevBuf<XlRun> d_xl_runs;
  DevBuf<XlHeader> d_xl_hdr;
  DevBuf<XlChunk> d_xl_chunks;
  DevBuf<uint32_t> d_xl_idx;
  // ks_integrate_round_exact (ks_k_shard.h).  A MARCHER context: frame_tail ends with the frame's updates as records grouped by
  // owner (sh_out[*]), nothing is applied; an OWNER context: scratch for the records of one frame of a round.
  bool shard_export = false;
  int shard_world = 1;
  uint64_t shard_frames_seen = 0;        // global frames this marcher has accounted for (its own, and empty ones for the other ranks')
  DevBuf<uint64_t> d_sh_okey[2];
  DevBuf<uint64_t> d_sh_gkey[2];
  DevBuf<uint32_t> d_sh_seq[2];
  DevBuf<float> d_sh_sdf[2];
  DevBuf<float> d_sh_uw[2];
  DevBuf<uint32_t> d_sh_counts;          // [64] per owner + [64] the origin-voxel flag
  size_t cap_sh = 0;
  uint32_t sh_counts[65] = {0};          // the last exported frame's
  uint64_t sh_exported = 0;              // its update count
  DevBuf<uint64_t> d_sh_tk;              // owner: tile keys / pair keys / record numbers of the segment being applied
  DevBuf<uint64_t> d_sh_pairs[2];
  DevBuf<uint32_t> d_sh_vals[2];
  size_t cap_sh_rx = 0;
  // ... of `merged` (ks_k_shard_merged.h).  Marcher: bundle number by position, the frame's bundle table, its mixed-label rows
  DevBuf<uint32_t> d_shm_bno;
  DevBuf<float2> d_shm_btab;
  DevBuf<uint32_t> d_shm_mpos;
  DevBuf<uint32_t> d_shm_cnt;            // [0] bundles, [1] mixed-label bundles
  size_t cap_shm_n = 0;                  // of the four above
  DevBuf<float> d_shm_mixed;             // [mixed-label bundles x kNumLabels]
  uint32_t shm_counts[2] = {0, 0};       // the last exported frame's
  // owner: the tables received from the peers (one after the other, by source rank), the staged operands, the long runs
  DevBuf<float2> d_shm_rx_btab;
  DevBuf<float> d_shm_rx_mixed;          // [rows x kNumLabels]
  DevBuf<float4> d_shm_ops;
  DevBuf<uint32_t> d_shm_long;           // [cap / (kLongRun + 1) + 1] heads of the long runs, then the count
  size_t cap_shm_ops = 0;                // of the two above
  // the runs of 33 .. 1024 updates a lane per run, bucketed by length over the frame (k_apply_long_lanes); by parity, like the lists
  bool long_lanes = true;
  unsigned long long long_lanes_min_pairs = 1ull << 24;
  DevBuf<unsigned long long> d_long_sorted_[2];
  DevBuf<LongHdr> d_long_hdr_[2];
  DevBuf<unsigned long long> d_xl_fb;
  uint32_t cap_xl_chunks = 1u << 17;   // 8 M updates in such runs per frame (more: the serial kernel takes the rest)
  // ks_mesh_update (ks_k_mesh.h).  The mesh lives in one of two arenas as per-block segments back to back; a call writes the
  // other arena (re-meshed blocks from the kernels, kept ones copied) and swaps.  The host keeps the directory and the
  // sorted block list: between two removals tiles only join a map, so the list is extended by the tiles that are new since the
  // last call; a removal (remove_tiles) brings the list up to date itself, takes its blocks out and restarts the count.
  MeshArena mesh_arena[2] = {};            // views of the four owners below
  DevBuf<float> mesh_xyz[2], mesh_nrm[2];
  DevBuf<uint32_t> mesh_rgba[2];
  DevBuf<uint8_t> mesh_label[2];
  size_t mesh_cap[2] = {0, 0};
  int mesh_cur = 0;
  bool mesh_valid = false;                 // false: the next call meshes everything, whatever only_stale says
  float mesh_min_weight = 0.f;             // ... as does a call with another min_weight than the stored mesh was made with
  std::vector<uint64_t> mesh_blocks;       // packed (x, y, z) of every block of the map, ascending
  uint32_t mesh_tiles_seen = 0;            // tiles [0, seen) have entered mesh_blocks
  std::vector<ks_mesh_block> mesh_dir;     // one entry per element of mesh_blocks as of the last update (n_vertices may be 0)
  std::vector<int32_t> mesh_changed;       // blocks whose segment the last update replaced
  DevBuf<uint8_t> d_mesh_buf[10];          // grow-only scratch of the passes (mesh_scratch)
  // ks_mesh_index (ks_k_mesh_index.h): the indexed view of the stored mesh, a snapshot that the next ks_mesh_update or clear drops.
  // Work space and outputs follow the corner count of the stored mesh (grow-only), never the map.
  DevBuf<uint32_t> mi_key32[2], mi_val[2]; // sort 1 (z) and the payloads; afterwards run numbers | corner flags, and the first corners
  DevBuf<uint64_t> mi_key64[2];            // sort 2 (x, y)
  DevBuf<uint32_t> mi_partial, mi_counts;  // the scans' slice sums; {vertices, largest valence, runs}
  DevBuf<float> mi_xyz, mi_nrm;            // the indexed mesh: per vertex ...
  DevBuf<uint32_t> mi_rgba, mi_obj, mi_valence;
  DevBuf<uint8_t> mi_label;
  DevBuf<uint32_t> mi_indices;             // ... and per corner
  bool mi_valid = false;
  size_t mi_corners = 0, mi_vertices = 0;
  // ks_esdf_update / ks_esdf_refresh (ks_k_esdf.h).  The store holds 512 records per tile slot: the ESDF of the map as it
  // was at the last update or refresh; the buffers grow only.  A removal moves the records with their tiles and lowers
  // esdf_tiles to the new tile count (remove_tiles).
  DevBuf<EsdfRecord> esdf_store;           // [esdf_tiles][512]
  DevBuf<uint64_t> esdf_keys[2];           // the two key buffers of the passes: [sign][box voxel] each
  DevBuf<uint32_t> esdf_slots;             // dense slot grid of the box
  DevBuf<unsigned long long> esdf_counters;
  DevBuf<EsdfRecord> esdf_out;             // staging of download and query
  DevBuf<int32_t> esdf_idx;
  DevBuf<float> esdf_xyz;
  bool esdf_valid = false;                 // an update has run since the map was last cleared
  uint32_t esdf_tiles = 0;                 // tiles that were resident at that update (or at the last refresh)
  ks_esdf_config esdf_cfg{};               // of the update that made the stored ESDF: what a refresh recomputes with
  uint64_t esdf_totals[3] = {0, 0, 0};     // voxels observed | fixed | clamped of the whole store
  std::vector<int32_t> esdf_changed;       // blocks that hold a tile the last refresh recomputed
  DevBuf<uint64_t> esdf_bricks[2];         // refresh: the bricks of lists X and Y
  DevBuf<uint64_t> esdf_lists;             // ... the sorted positions of X | Y | Z
  DevBuf<uint32_t> esdf_zslots;            // ... the pool slot of each position of Z
  // ks_esdf_sample / ks_esdf_slice / ks_esdf_sweep (ks_k_esdf_read.h): the counters, and what the host-pointer calls stage per chunk
  DevBuf<unsigned long long> esdf_read_counters;
  DevBuf<float> esdf_read_in, esdf_read_f;   // points or segments in; distance | gradient, or t_stop | min_clearance | t_min out
  DevBuf<uint8_t> esdf_read_b;             // status | label | flags
  size_t esdf_read_chunk = size_t(1) << 20;   // points, segments or pixels staged at a time
  // ks_render_view (ks_k_render.h): the images of the host-pointer call before they are copied out, and the three counters
  DevBuf<float> render_depth, render_normals;
  DevBuf<uint32_t> render_rgba;
  DevBuf<uint8_t> render_labels;
  DevBuf<unsigned long long> render_counters;
  // ks_align_points (ks_k_align.h): the wavefronts' partial sums, the state block, and the cloud of the host-pointer call
  DevBuf<double> align_partials;
  DevBuf<AlignState> align_state;
  DevBuf<float> align_xyz;
  // ks_objects_update (ks_k_objects.h).  The id store holds 512 words per tile slot: the objects of the map as it was at the last
  // update; the buffers grow only.  A removal moves the ids with their tiles and lowers obj_tiles to the new tile count.
  DevBuf<uint32_t> obj_ids;                // [obj_tiles][512] (during an update: the provisional numbers of the roots)
  DevBuf<uint32_t> obj_parent;             // the union-find forest of an update, then the voxels' provisional numbers
  DevBuf<uint8_t> obj_cls;                 // the class byte of every voxel
  DevBuf<ObjCounters> obj_counters;
  DevBuf<ObjAcc> obj_acc;                  // per provisional component
  DevBuf<uint64_t> obj_keys[2];            // the sort's key and payload buffers
  DevBuf<uint32_t> obj_vals[2];
  DevBuf<uint32_t> obj_final;              // provisional number -> object index
  DevBuf<ks_object> obj_records;
  DevBuf<uint32_t> obj_out;                // staging of download and query
  DevBuf<int32_t> obj_idx;
  DevBuf<float> obj_xyz;
  bool obj_valid = false;                  // an update has run since the map was last cleared
  uint32_t obj_tiles = 0;                  // tiles that were resident at that update
  size_t obj_count = 0;                    // records stored
  // ks_nav_update (ks_k_nav.h).  The field holds 512 words per tile slot of the ESDF store it was made from: a snapshot that the
  // next ESDF update or refresh, a removal or a clear drops; the buffers grow only.
  DevBuf<uint32_t> nav_cost;               // [nav_tiles][512]
  DevBuf<uint32_t> nav_lists;              // [2][nav_tiles]: the active tiles of this round and of the next
  DevBuf<uint32_t> nav_queued;             // [nav_tiles] the tile waits on a list, then the three rotating list counts
  DevBuf<NavCounters> nav_counters;
  DevBuf<unsigned long long> nav_path_counters;
  DevBuf<float> nav_in, nav_wp;            // goals, or the starts of a chunk; the waypoints of a chunk
  DevBuf<uint32_t> nav_u32;                // staging of query, download and paths (cost | n_waypoints)
  DevBuf<uint8_t> nav_u8;                  // ... the path statuses
  DevBuf<int32_t> nav_idx;
  bool nav_valid = false;
  uint32_t nav_tiles = 0;
  size_t nav_chunk = size_t(1) << 20;      // points or starts staged at a time
  // ks_frontiers_update (ks_k_frontier.h).  The id store holds 512 words per tile slot of the ESDF store it was made from: a
  // snapshot with the lifetime of the navigation field (drop_frontiers); the buffers grow only.
  DevBuf<uint32_t> fr_ids;                 // [fr_tiles][512] (during an update: the provisional numbers of the roots)
  DevBuf<uint32_t> fr_parent;              // the union-find forest of an update, then the voxels' provisional numbers
  DevBuf<uint8_t> fr_cls, fr_faces;        // the class byte and the unknown-face count of every voxel
  DevBuf<unsigned long long> fr_planes;    // [fr_tiles][8][observed | candidate]: 128 B per tile
  DevBuf<ObjCounters> fr_numbered;         // k_obj_number's component count
  DevBuf<FrCounters> fr_counters;
  DevBuf<FrAcc> fr_acc;                    // per provisional component
  DevBuf<uint64_t> fr_keys[2];             // the sort's key and payload buffers
  DevBuf<uint32_t> fr_vals[2];
  DevBuf<uint32_t> fr_final;               // provisional number -> frontier index
  DevBuf<ks_frontier> fr_records;
  DevBuf<uint32_t> fr_out;                 // staging of download and query
  DevBuf<int32_t> fr_idx;
  DevBuf<float> fr_xyz;
  bool fr_valid = false;
  uint32_t fr_tiles = 0;
  size_t fr_count = 0;
  // ks_rooms_update (ks_k_rooms.h).  Two planes of 512 words per tile slot of the ESDF store they were made from, the records, the
  // links and the room of every object: a snapshot with the lifetime of the frontiers (drop_rooms); the buffers grow only.
  DevBuf<uint32_t> rooms_room, rooms_cost;    // [rooms_tiles][512] (rooms_room during an update: the provisional numbers of the roots)
  DevBuf<uint32_t> rooms_parent;              // the union-find forest of an update, then the voxels' provisional numbers
  DevBuf<uint8_t> rooms_cls;                  // the class byte of every voxel
  DevBuf<uint32_t> rooms_lists, rooms_queued; // the work lists of both relaxations, as nav_lists and nav_queued
  DevBuf<NavCounters> rooms_nav_counters;     // rounds and tile relaxations
  DevBuf<ObjCounters> rooms_numbered;         // k_obj_number's and k_obj_keys' counts
  DevBuf<RoomCounters> rooms_counters;
  DevBuf<ObjAcc> rooms_core_acc;              // per provisional component
  DevBuf<ks_object> rooms_cores;              // k_obj_records' records of the rooms' cores
  DevBuf<uint32_t> rooms_final;               // provisional number -> room
  DevBuf<RoomAcc> rooms_acc;                  // per room
  DevBuf<uint64_t> rooms_keys[2];             // the sorts' key and payload buffers: components, then contact pairs
  DevBuf<uint32_t> rooms_vals[2];
  DevBuf<uint64_t> rooms_head_keys[2];        // ... and the heads of the runs
  DevBuf<uint32_t> rooms_head_vals[2];
  DevBuf<RoomLinkAcc> rooms_link_acc;
  DevBuf<unsigned long long> rooms_obj_best;  // per object: the smallest cost << 32 | room of its voxels
  DevBuf<ks_room> rooms_records;
  DevBuf<ks_room_link> rooms_links;
  DevBuf<uint32_t> rooms_obj_room;            // the room of every object of the join
  DevBuf<uint32_t> rooms_out;                 // staging of download and query
  DevBuf<int32_t> rooms_idx;
  DevBuf<float> rooms_xyz;
  bool rooms_valid = false;
  uint32_t rooms_tiles = 0;
  size_t rooms_count = 0, rooms_link_count = 0, rooms_obj_count = 0;
  // ks_view_gain (ks_k_view_gain.h): nothing is stored between calls; the buffers grow only
  DevBuf<unsigned long long> vg_planes;    // [esdf_tiles][8][observed | occupied | labelled | 0]: 256 B per tile
  DevBuf<uint32_t> vg_slabs;               // [groups][slab_words]: the visited bitmaps of the views that do not fit the LDS
  DevBuf<VgCounters> vg_counters;
  DevBuf<float> vg_poses;                  // staging of the host entry
  DevBuf<ks_view_gain_record> vg_records;
  uint32_t vg_lds_bits = kVgLdsBits;       // KS_DEBUG=1 KS_VG_LDS_BITS=<n> (tests): the LDS budget in bits; 0: every view through global memory
  uint32_t vg_groups = kVgMaxGroups;       // KS_DEBUG=1 KS_VG_GROUPS=<n> (tests): workgroups in flight
  // ks_path_shorten (ks_k_path.h): nothing is stored between calls (the counters are esdf_read_counters); what the host entry stages
  DevBuf<float> ps_in, ps_out, ps_f;       // the waypoints of a chunk of paths in and out; length | min_clearance
  DevBuf<uint32_t> ps_u32;                 // n_waypoints in | out
  DevBuf<uint8_t> ps_u8;                   // the statuses
  size_t ps_chunk = size_t(1) << 20;       // KS_DEBUG=1 KS_SHORTEN_CHUNK=<paths> (tests): paths staged at a time
  uint32_t ps_blocks = 4096;               // KS_DEBUG=1 KS_SHORTEN_GRID=<workgroups> (tests): the bound of k_path_shorten's grid
  // ks_remove_blocks / ks_remove_distant_blocks (ks_k_remove.h).  What the stored products still have to hear of a removal:
  std::vector<int32_t> removed_blocks;     // the blocks the LAST removal call took out, ascending (ks_removed_blocks)
  std::vector<uint64_t> mesh_removed;      // block words removed since the last ks_mesh_update, ascending: it reports them as
                                           // changed and re-meshes the resident blocks whose border cubes read them
  std::vector<uint64_t> esdf_removed;      // tile positions (pack_coord3) removed since the stored ESDF was last brought up to date:
                                           // stale positions without a tile for ks_esdf_refresh
  DevBuf<uint8_t> rm_mark;                 // one byte per slot: the tile leaves
  DevBuf<uint64_t> rm_keys;                // the tile keys of the listed blocks
  DevBuf<uint2> rm_moves;                  // {source slot, destination slot} per moved tile
  // ks_fuse_map (ks_k_fuse.h), held by the DESTINATION context; grow-only
  DevBuf<uint4> fuse_ws;                   // the work space: one exchange-format tile (64 KiB) per candidate tile of a chunk
  DevBuf<uint64_t> fuse_keys;              // the chunk's candidate keys, then the keys of its touched tiles
  DevBuf<uint32_t> fuse_u32;               // per candidate its count of touched voxels, then offs and idx of k_merge_tiles
  ks_profile prof{};
  ProfSet pset[kProfSets];
  bool fatal = false;
};

#define HIPCHK(ctx, expr)                                                                         \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                             \
      return KS_ERR_HIP;                                                                          \
    }                                                                                             \
  } while (0)

// the stored frontiers are a snapshot of the ESDF store: they go wherever the navigation field goes
static void drop_frontiers(ks_ctx* c) {
  c->fr_valid = false;
  c->fr_count = 0;
}

// ... and so do the stored rooms
static void drop_rooms(ks_ctx* c) {
  c->rooms_valid = false;
  c->rooms_count = c->rooms_link_count = c->rooms_obj_count = 0;
}

int ks_hip_failed(ks_ctx* ctx, const char* what, hipError_t e) {
  ctx->err = std::string(what) + ": " + hipGetErrorString(e);
  return KS_ERR_HIP;
}

namespace {

inline hipStream_t march_stream(ks_ctx* c, uint64_t frame_no) { return c->stream_march_[frame_no % (uint64_t)c->n_march]; }
inline uint64_t* observed_table(ks_ctx* c, uint64_t frame_no) { return c->d_observed_[frame_no % (uint64_t)c->n_obs]; }
int sync_march(ks_ctx* c) {
  for (int i = 0; i < c->n_march; ++i)
    if (c->stream_march_[i] != c->stream) HIPCHK(c, hipStreamSynchronize(c->stream_march_[i]));
  return KS_OK;
}

// Rehash schedule of the host's libstdc++ unordered_map (the container the reference keeps its bundles in,
// [K:include/kimera_semantics/common.h:37]): probed from a real container, once, up to the element count needed.
void probe_rehash_schedule(size_t n_max, BoSchedule* out) {
  static std::mutex mu;
  static std::vector<uint32_t> t, b;
  static size_t probed = 0;
  std::lock_guard<std::mutex> lk(mu);
  if (probed < n_max) {
    t.clear();
    b.clear();
    std::unordered_map<uint32_t, char> m;
    size_t bc = m.bucket_count();
    for (uint32_t i = 0; i < n_max; ++i) {
      m.emplace(i, 0);
      if (m.bucket_count() != bc) {  // inserting element i took over a new bucket array
        bc = m.bucket_count();
        t.push_back(i);
        b.push_back((uint32_t)bc);
      }
    }
    probed = n_max;
  }
  *out = BoSchedule{};
  uint32_t off = 0;
  int e = 0;
  for (; e < (int)t.size() && e < kBoMaxEpochs && t[e] < n_max; ++e) {
    out->t[e] = t[e];
    out->b[e] = b[e];
    out->head_off[e] = off;
    off += b[e];
  }
  out->n_epochs = (uint32_t)e;
  out->t[e] = UINT32_MAX;
}

int ensure_bundle_order(ks_ctx* c, size_t cap) {
  probe_rehash_schedule(cap, &c->bo_sched);
  const BoSchedule& S = c->bo_sched;
  {
    // The closed form of the iteration order (ks_k_bundle_order.h) is that of libstdc++'s unordered_map — the container the
    // reference is built with — and k_bo_small knows its tenth bucket count.  A library built against another standard
    // library (another prime policy) would compute some other, self-consistent order: refuse instead.
    static const uint32_t kLibstdcxxBuckets[] = {13, 29, 59, 127, 257, 541, 1109, 2357, 5087, 10273, 20753, 42043, 85229, 172933};
    for (uint32_t e = 0; e < S.n_epochs && e < sizeof(kLibstdcxxBuckets) / sizeof(uint32_t); ++e)
      if (S.b[e] != kLibstdcxxBuckets[e] || (e > 0 && S.t[e] != kLibstdcxxBuckets[e - 1])) {
        c->err = "bundle_order = KS_BUNDLE_ORDER_REFERENCE needs libstdc++'s unordered_map rehash schedule (13, 29, 59, ...): this build's standard "
                 "library differs; use KS_BUNDLE_ORDER_CANONICAL";
        return KS_ERR_UNSUPPORTED;
      }
  }
  c->bo_epochs = (int)S.n_epochs;
  size_t heads = 0;
  for (uint32_t e = 0; e < S.n_epochs; ++e) heads += S.b[e];
  const size_t nbt = cap / kBoBlock + 2, nfbt = 2 * cap / kBoBlock + 2;
  auto al = [](size_t words) { return (words * 4 + 255) & ~(size_t)255; };
  const size_t per_map = 11 * al(cap) + al(nbt) + al(heads);
  const size_t total = 2 * per_map + al(2) + al((sizeof(BoSchedule) + 3) / 4) + 2 * al(2 * cap) + al(nfbt) + al(cap);
  if (int rc = c->d_bo_slab.alloc(c, total)) return rc;
  uint8_t* p = c->d_bo_slab;
  auto take = [&](size_t words) { uint32_t* r = (uint32_t*)p; p += al(words); return r; };
  for (int m = 0; m < 2; ++m) {
    BoMap& M = c->bo.m[m];
    M.H = take(cap); M.rank = take(cap);
    M.next[0] = take(cap); M.next[1] = take(cap);
    M.idj[0] = take(cap); M.idj[1] = take(cap);
    M.kj[0] = take(cap); M.kj[1] = take(cap);
    M.lp = take(cap); M.gm = take(cap); M.cj = take(cap);
    M.bt = take(nbt);
    M.head = take(heads);
    HIPCHK(c, hipMemsetAsync(M.head, 0xff, heads * 4, c->stream));  // chains are empty between frames
  }
  c->bo.B = take(2);
  BoSchedule* d_sched = (BoSchedule*)take((sizeof(BoSchedule) + 3) / 4);
  c->bo.sched = d_sched;
  c->bo.flag = take(2 * cap);
  c->bo.flag_lp = take(2 * cap);
  c->bo.flag_bt = take(nfbt);
  c->bo.t_of_head = take(cap);
  HIPCHK(c, hipMemcpyAsync(d_sched, &c->bo_sched, sizeof(BoSchedule), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KS_OK;
}

// chains of the ordered-phase schedule = the groups of the frame's integration order (ks_types.h: FrameParams::chains)
inline uint32_t order_chains(int order_mode, size_t n) {
  const size_t q = n / kOrderStep;
  return (order_mode == KS_ORDER_MIXED && q >= 1) ? (uint32_t)q : kOrderStep;
}
// ... and what a frame of at most `cap` points can reach: stage B's launches are sized by the slot's capacity
inline uint32_t order_chains_cap(int order_mode, size_t cap) { return std::max(order_chains(order_mode, cap), order_mode == KS_ORDER_MIXED ? kOrderStep : 0u); }
inline uint32_t order_generations_cap(int order_mode, size_t cap) {
  // KS_ORDER_MIXED: n / (n / 1024) < 2048 generations for every n >= 1024; one generation below that.
  // The other orders: 1024 chains, ceil(n / 1024) generations.
  if (order_mode == KS_ORDER_MIXED) return cap >= kOrderStep ? 2u * kOrderStep - 1u : 1u;
  return (uint32_t)((cap + kOrderStep - 1) / kOrderStep);
}
// phase boundaries (in generations: one integration position per chain) of the ordered-phase early-out
std::vector<uint32_t> phase_bounds(uint32_t n_gen, int growth) {
  std::vector<uint32_t> b{0};
  for (;;) {
    const uint64_t inc = std::max<uint64_t>(1, (uint64_t)b.back() * (uint64_t)(growth - 16) / 16);
    if (b.back() + inc >= n_gen) break;
    b.push_back((uint32_t)(b.back() + inc));
  }
  return b;
}
// (chain, sub-run) pairs that EXIST in phase [g0, g1) of a frame of n points — those with at least one integration position
// below n; the ones that hold a live ray (the items of k_seed_list) are among them
inline uint64_t seed_items_of(int order_mode, size_t n, uint32_t g0, uint32_t g1) {
  if (n == 0) return 0;
  const uint64_t chains = order_chains(order_mode, n), full = n / chains, part = n % chains;   // `part` chains reach one generation further
  auto subs = [&](uint64_t gens) -> uint64_t {
    const uint64_t hi = std::min<uint64_t>(g1, gens);
    return hi > g0 ? (hi - g0 + kSubRun - 1) / kSubRun : 0;
  };
  return (chains - part) * subs(full) + part * subs(full + 1);
}
// The seed's launch shape for a slot of `cap` points: the phases of the capacity's generation count, and per phase the most
// items ANY frame of at most cap points can have in it (item_cap = wavefronts launched per frame; 0 = no frame reaches the
// phase, nothing is launched).  The chain count and the generation count never peak together — in the default order a
// frame of n points has n / 1024 chains and fewer than 1024 + 1024 / (n / 1024) + 1 generations — so this is far below their
// product.  For a given chain count the items grow with n: the maximum is taken over the largest frame of every chain count.
std::vector<SeedPhase> seed_launch_shape(int order_mode, int growth, size_t cap) {
  const uint32_t n_gen = order_generations_cap(order_mode, cap);
  const std::vector<uint32_t> B = phase_bounds(n_gen, growth);
  std::vector<SeedPhase> out;
  uint64_t off = 0;
  for (size_t j = 0; j < B.size(); ++j) {
    const uint32_t g0 = B[j], g1 = (j + 1 < B.size()) ? B[j + 1] : n_gen;
    uint64_t m = 0;
    if (order_mode == KS_ORDER_MIXED) {
      m = seed_items_of(order_mode, std::min<size_t>(cap, kOrderStep - 1), g0, g1);   // fewer than 1024 points: one generation of them
      for (size_t q = 1; q <= cap / kOrderStep; ++q) m = std::max(m, seed_items_of(order_mode, std::min<size_t>(cap, q * kOrderStep + kOrderStep - 1), g0, g1));
    } else {
      m = seed_items_of(order_mode, cap, g0, g1);   // 1024 chains whatever n
    }
    out.push_back(SeedPhase{g0, g1, (uint32_t)off, (uint32_t)m});
    off += m;
  }
  return out;
}

// longest possible ray of a frame of this context, in voxels
size_t steps_max_of(const ks_config& cfg, float voxel_size_inv) {
  const double max_len = (double)cfg.max_ray_length_m + 2.0 * (double)cfg.truncation_distance;
  return (size_t)std::ceil(1.7321 * max_len * (double)voxel_size_inv) + 8;
}
int ensure_exact_points(ks_ctx* c, size_t cap);
int ensure_points(ks_ctx* c, size_t n) {
  if (n <= c->cap_points) return KS_OK;
  // the create-time size is exact; a cloud that outgrows it gets head-room (growing completes the frames in
  // flight and re-captures stage B)
  const size_t cap = std::max<size_t>(c->cap_points ? n + n / 8 : n, 1024);
  c->cap_points = 0;   // (of the whole group below: a failure part-way leaves a context that allocates again, not one that trusts the old size)
  int rc;
  if ((rc = c->d_xyz.alloc(c, cap * 3))) return rc;
  if ((rc = c->d_rgba.alloc(c, cap * 4))) return rc;
  if ((rc = c->d_labels.alloc(c, cap))) return rc;
  ++c->buffers_epoch;
  const size_t scan_cap = (c->cfg.method == KS_METHOD_MERGED ? 2 : 1) * cap;
  size_t seed_items = 0;
  if (c->uses_early_out) {
    // the seed's launch shape and work-list sizes follow the capacity (the captured stage-B graphs are keyed by it)
    c->seed_phases = seed_launch_shape(c->cfg.integration_order_mode, c->cfg.early_out_phase_growth, cap);
    uint32_t off = 0;
    for (SeedPhase& P : c->seed_phases) {
      // (the fields of an item word, ks_k_march.h: nowhere near with the 2^22 points the early-out's marks allow)
      if ((P.g1 - P.g0 + kSubRun - 1) / kSubRun > (1u << kSeedSubBits) || order_chains_cap(c->cfg.integration_order_mode, cap) > (1u << kSeedChainBits)) {
        c->err = "point cloud too large for the early-out's work list";
        return KS_ERR_INVALID_ARG;
      }
      if (c->seed_cap_items) P.item_cap = (uint32_t)std::min<size_t>(P.item_cap, c->seed_cap_items);
      P.item_off = off;
      off += P.item_cap;
    }
    seed_items = off;
    if ((rc = c->d_seed_phases.alloc(c, c->seed_phases.size()))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_seed_phases, c->seed_phases.data(), c->seed_phases.size() * sizeof(SeedPhase), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  for (int i = 0; i < (c->cfg.pipeline_frames ? c->n_slots : 1); ++i) {
    if (c->uses_early_out) {
      // (one generation of slack: a frame's last generation may be partial)
      if ((rc = c->slot[i].d_seed_gen.alloc(c, cap + order_chains_cap(c->cfg.integration_order_mode, cap)))) return rc;
      if ((rc = c->slot[i].d_seed_items.alloc(c, seed_items))) return rc;
      if ((rc = c->slot[i].d_seed_n.alloc(c, c->seed_phases.size()))) return rc;
    }
    if ((rc = c->slot[i].d_rays.alloc(c, cap))) return rc;
    if ((rc = c->slot[i].d_ray_list.alloc(c, cap))) return rc;
    if ((rc = c->slot[i].d_cnt.alloc(c, scan_cap))) return rc;
    if ((rc = c->slot[i].d_lp.alloc(c, scan_cap))) return rc;
    if ((rc = c->slot[i].d_bt.alloc(c, scan_cap / kScanBlock + 2))) return rc;
    if (c->cfg.method == KS_METHOD_FAST && (rc = c->slot[i].d_live.alloc(c, cap))) return rc;
    if (c->cfg.enable_anti_grazing && c->cfg.method == KS_METHOD_MERGED) {
      if ((rc = c->slot[i].d_gkeys.alloc(c, cap))) return rc;
      if ((rc = c->slot[i].d_rkeys.alloc(c, cap))) return rc;
    }
    if (c->cfg.method == KS_METHOD_MERGED && (rc = c->slot[i].d_deltas.alloc(c, cap * kNumLabels))) return rc;
  }
  if ((rc = c->d_hash.alloc(c, cap))) return rc;
  if ((rc = c->d_skeys32.alloc(c, cap))) return rc;
  if ((rc = c->d_skeys32b.alloc(c, cap))) return rc;
  if ((rc = c->d_pkeys.alloc(c, cap))) return rc;
  if ((rc = c->d_pkeys2.alloc(c, cap))) return rc;
  if ((rc = c->d_pvals.alloc(c, cap))) return rc;
  if ((rc = c->d_pvals2.alloc(c, cap))) return rc;
  if ((rc = c->d_order.alloc(c, cap))) return rc;
  if ((rc = c->d_inv_order.alloc(c, cap))) return rc;
  if ((rc = c->d_okeys.alloc(c, cap))) return rc;
  if ((rc = c->d_okeys2.alloc(c, cap))) return rc;
  if ((rc = c->d_ovals.alloc(c, cap))) return rc;
  if (c->cfg.method == KS_METHOD_MERGED) {
    if ((rc = c->d_gpw.alloc(c, cap))) return rc;
    if ((rc = c->d_glc.alloc(c, cap))) return rc;
    if ((rc = c->d_ray_keys.alloc(c, cap))) return rc;
    if ((rc = c->d_blong.alloc(c, cap / kLongRun + 64))) return rc;
    if (c->key_bits) {
      size_t slots = 1024;
      while (slots < 2 * cap) slots <<= 1;
      if ((rc = c->d_key_overflow.alloc(c, slots))) return rc;
      HIPCHK(c, hipMemsetAsync(c->d_key_overflow, 0, slots * sizeof(uint64_t), c->stream));
      c->key_overflow_mask = (uint32_t)(slots - 1);
    }
  }
  if (c->use_bundle_rank && (rc = ensure_bundle_order(c, cap))) return rc;
  if (c->exact_early_out) {
    if ((rc = c->d_eo_lp.alloc(c, cap))) return rc;
    if ((rc = c->d_eo_bt.alloc(c, cap / kScanBlock + 2))) return rc;
    if ((rc = ensure_exact_points(c, cap))) return rc;
  }
  c->cap_points = cap;
  return KS_OK;
}

// d_pairs is written by k_emit before the host knows the pair count: it is sized from what earlier
// frames needed (+25 %); a frame that does not fit raises kErrPairs instead of writing, and its tail
// grows the buffer and repeats the emission (frame_tail).  d_pairs2 / the long-run list are sized by
// the actual count.
int ensure_pairs_in(ks_ctx* c, FrameSlot& S, size_t bound) {
  if (bound <= S.d_pairs.size()) return KS_OK;
  if (int rc = S.d_pairs.alloc(c, std::max<size_t>(bound, 1 << 20))) return rc;
  ++c->buffers_epoch;  // captured stage-B graphs point at the old buffer
  return KS_OK;
}
int ensure_pairs_out(ks_ctx* c, size_t n) {
  if (n <= c->cap_pairs) return KS_OK;
  const size_t cap = std::max<size_t>(n + n / 4, 1 << 20);
  c->cap_pairs = 0;
  int rc;
  HIPCHK(c, hipStreamSynchronize(c->stream_long));  // long runs of the previous frame may still read them
  if (c->stream_xlong) HIPCHK(c, hipStreamSynchronize(c->stream_xlong));
  if (c->stream_tail) HIPCHK(c, hipStreamSynchronize(c->stream_tail));
  for (int b = 0; b < 2; ++b) {
    if ((rc = c->d_pairs2_[b].alloc(c, cap))) return rc;
    // heads of the long runs, then (from cap / kLongRunLanes + 64 on) the heads of the runs of more than kXLongRun updates
    if ((rc = c->d_long_list_[b].alloc(c, cap / kLongRunLanes + 64 + cap / kXLongRun + 64))) return rc;
    if (c->long_lanes && (rc = c->d_long_sorted_[b].alloc(c, cap / kLongRunLanes + 64))) return rc;
  }
  if (c->d_xl_hdr && (rc = c->d_xl_fb.alloc(c, cap / kXLongRun + 64))) return rc;   // (the runs the integer-sum path leaves to k_apply_xlong)
  c->cap_pairs = cap;
  return KS_OK;
}

template <typename K>
int sort_keys(ks_ctx* c, K* a, K* b, size_t n, unsigned end_bit, K** result, unsigned begin_bit = 0, bool tail = false) {
  HIPCHK(c, (ksrs::sort<K, false>(tail ? c->sort_ws_tail : c->sort_ws, a, b, nullptr, nullptr, n, end_bit,
                                  tail ? c->stream_tail : c->stream, result, nullptr, begin_bit)));
  return KS_OK;
}
template <typename K>
int sort_pairs(ks_ctx* c, K* ka, K* kb, uint32_t* va, uint32_t* vb, size_t n, unsigned end_bit, K** kres,
               uint32_t** vres, unsigned begin_bit = 0) {
  HIPCHK(c, (ksrs::sort<K, true>(c->sort_ws, ka, kb, va, vb, n, end_bit, c->stream, kres, vres, begin_bit)));
  return KS_OK;
}

inline unsigned bits_for(uint64_t n) {  // number of bits needed to represent values < n
  unsigned b = 1;
  while (b < 64 && (1ull << b) < n) ++b;
  return b;
}

// Bits of a pair key's sequence field that hold the frame's index in its batch, above the ray sequence (0: this context's
// keys have none).  `fast` contexts that launch stage B per batch: the tail of such a batch sorts and applies the pairs of all
// its frames in one pass (tail_batch), and the stable sort, which skips the sequence field, leaves every voxel's updates in
// (frame, integration position) order.  The field then has the same width for every frame — that of the slot capacity, not of
// the frame's own point count — and must leave room for the 9 + 23 bits of the largest voxel id under the key's info byte.
inline unsigned tail_frame_bits(const ks_ctx* c) {
  if (c->batch <= 1 || c->cfg.method != KS_METHOD_FAST || c->shard_export) return 0u;
  const unsigned fb = bits_for((uint64_t)c->batch);
  return bits_for(c->cap_points) + fb + 9u + 23u <= 56u ? fb : 0u;
}
int launch_batch(ks_ctx* c);
int quiesce(ks_ctx* c);
// ApproxHashSet::resetApproxSet.  `observed`: the early-out set, whose entries carry a frame tag
// (ks_k_march.h); its poison value and tag bookkeeping differ from the start-voxel set's raw hashes.
int reset_set(ks_ctx* c, uint64_t* d_set0, uint64_t* offset, bool observed) {
  const bool full = ++(*offset) >= kFullResetThreshold;
  // entries written before this offset bump can never match again; when the 10-bit frame tag is about
  // to run out they are retired in one pass and the tags start over
  const bool retag = observed && !full && c->obs_tag + (uint32_t)c->cfg.clear_checks_every_n_frames + 2u >= kObsMaxTag;
  if (full || retag) {
    // frames whose stage B still waits for its batch to fill carry the OLD tag / offset in their FrameParams: they go
    // out before the tables are rewritten (a frame with tag ~1019 running after the retag would leave marks that win
    // every atomicMax against the restarted tags 1, 2, ...)
    if (int rc = launch_batch(c)) return rc;
    if (full && c->exact_early_out) {
      // the table the exact mode keeps verbatim is rewritten below: a frame in flight whose device fix point gave up repeats
      // it on the tail stream LATER, reading and committing into that table — complete every pending tail first
      if (int rc = quiesce(c)) return rc;
    }
    if (int rc = sync_march(c)) return rc;  // stage B reads the observed set
    if (full) *offset = 0;
    for (int t = 0; t < (observed ? c->n_obs : 1); ++t) {
      uint64_t* d_set = observed ? c->d_observed_[t] : d_set0;
      if (full) {
        HIPCHK(c, hipMemsetAsync(d_set, 0, (observed ? 2 : 1) * (sizeof(uint64_t) << kSetBits), c->stream));
        const uint64_t poison = observed ? kObsPoison : ~0ull;
        HIPCHK(c, hipMemcpyAsync(d_set, &poison, sizeof(poison), hipMemcpyHostToDevice, c->stream));
      } else {
        hipLaunchKernelGGL(k_obs_retag, dim3((2u << kSetBits) / 256), dim3(256), 0, c->stream, d_set);
      }
    }
    if (observed && full && c->d_eo_plain) {  // resetApproxSet's full reset of the table the exact mode keeps verbatim
      HIPCHK(c, hipMemsetAsync(c->d_eo_plain, 0, sizeof(uint64_t) << kSetBits, c->stream));
      const uint64_t poison = ~0ull;
      HIPCHK(c, hipMemcpyAsync(c->d_eo_plain, &poison, sizeof(poison), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (observed) c->obs_tag = 0;
  }
  if (observed) c->obs_tag_lo = c->obs_tag + 1;  // the offset generation that starts with the coming frame
  return KS_OK;
}

inline void stage_mark(ks_ctx* c, int set, int ev) {
  if (set >= 0 && c->pset[set].stages)
    (void)hipEventRecord(c->pset[set].ev[ev], ev <= 3 ? c->stream : ev <= 5 ? c->prof_march_stream : c->stream_tail);
}

// fold a finished event set into ks_profile
void resolve_prof(ks_ctx* c, int set) {
  ProfSet& P = c->pset[set];
  if (!P.used || !P.complete) return;
  (void)hipEventSynchronize(P.ev[kStageEvents - 1]);
  if (P.stages) {
    for (int s = 0; s < KS_STAGE_COUNT; ++s) {
      float ms = 0.f;
      const int a = s < 3 ? s : s == 3 ? 4 : s + 2;
      if (hipEventElapsedTime(&ms, P.ev[a], P.ev[a + 1]) == hipSuccess) {
        c->prof.ms[s] += ms;
        c->prof.launches[s] += 1;
      }
    }
  }
  if (P.applied) {
    float kms = 0.f;
    if (hipEventElapsedTime(&kms, P.k0, P.k1) == hipSuccess) {
      c->prof.apply_kernel_ms += kms;
      c->prof.apply_kernel_launches += 1;
      c->prof.apply_kernel_updates += P.n_applied;
    }
  }
  c->prof.frames += 1;
  c->prof.updates += P.n_pairs;
  c->prof.points += P.n_points;
  P.used = P.complete = P.applied = false;
}

// what stage B's kernels see of a frame slot (ks_k_march.h)
SlotView slot_view(const FrameSlot& S, Counters* counters = nullptr) {
  SlotView v{};
  v.F = S.d_F;
  v.rays = S.d_rays;
  v.cnt = S.d_cnt;
  v.lp = S.d_lp;
  v.bt = S.d_bt;
  v.ray_list = S.d_ray_list;
  v.pairs = S.d_pairs;
  v.pairs_cap = (unsigned long long)S.d_pairs.size();
  v.C = counters ? counters : S.d_counters;
  v.host_snap = (uint32_t*)S.h_snap.get();
  v.eo_stats = S.d_eo_ctl ? &S.d_eo_ctl->n_x : nullptr;
  v.seed_gen = S.d_seed_gen;
  v.seed_items = S.d_seed_items;
  v.seed_n = S.d_seed_n;
  return v;
}

// pair emission over an upper bound of rays (<= n); the live ray count stays on the device
void launch_emit(ks_ctx* c, const BatchView& V, uint32_t nb, bool wide, hipStream_t st) {
  // grids and LDS are sized by the slot's capacity (the kernels take the frame's own counts from its d_F and its
  // counters): the launch sequence is the same for every frame and can be replayed
  const size_t n = c->cap_points;
  const size_t lds = ((2 * n + kScanBlock - 1) / kScanBlock) * sizeof(unsigned long long);
  if (!(c->cfg.method == KS_METHOD_MERGED && c->cfg.enable_anti_grazing)) {
    // bundles and 2 cm rays are long: 8 rays per wavefront; early-out rays are short: one per lane
    if (wide || c->cfg.method == KS_METHOD_MERGED || !c->uses_early_out) {
      hipLaunchKernelGGL(k_emit_lane<8>, dim3((uint32_t)((n + 31) / 32), nb), dim3(256), lds, st, V, c->table, c->pool);
    } else {
      hipLaunchKernelGGL(k_emit_lane<16>, dim3((uint32_t)((n + 63) / 64), nb), dim3(256), lds, st, V, c->table, c->pool);
    }
  } else if (wide) {
    hipLaunchKernelGGL(k_emit<64>, dim3((uint32_t)((n + 3) / 4), nb), dim3(256), lds, st, V, c->table, c->pool);
  } else {
    hipLaunchKernelGGL(k_emit<16>, dim3((uint32_t)((n + 15) / 16), nb), dim3(256), lds, st, V, c->table, c->pool);
  }
}

// Stage B of the nb frames of a batch, as a sequence of launches on stream sm (captured into a graph by the caller,
// or issued directly): every kernel covers the whole batch (blockIdx.y = frame).  Everything frame-specific comes
// from the slots' d_F.
// part: 0 = all of it; 1 = the early-out phases only; 2 = everything after them (the exact early-out mode runs its
// fix-point iteration, with host waits, in between)
void enqueue_stage_b(ks_ctx* c, const BatchView& V, uint32_t nb, bool wide, hipStream_t sm, size_t steps_max, int part = 0) {
  const ks_config& cfg = c->cfg;
  const size_t n = c->cap_points;  // NOT the frame's point count: see launch_emit
  if (c->uses_early_out && part != 2) {
    // ordered-phase early-out: per phase, k_test decides how far the phase's rays get against the set as it
    // stood when the phase began and enters their marks (ks_k_march.h).  One wavefront per item of the phase's work list
    // (built by stage A: k_seed_list, frame_front); the launch covers what a frame of the slot's capacity can have (seed_launch_shape),
    // a phase no such frame reaches is not launched, and k_test ends the frame's last phase at ITS n.
    for (size_t j = 0; j < c->seed_phases.size(); ++j) {
      const SeedPhase& P = c->seed_phases[j];
      if (P.item_cap == 0) continue;
      const uint32_t steps_cap = (uint32_t)((steps_max + 3) & ~(size_t)3);
      const size_t lds_wave = (size_t)test_lds_words64(steps_cap) * sizeof(unsigned long long);
      const uint32_t wpb = lds_wave * 4 <= 60 * 1024 ? 4u : lds_wave * 2 <= 60 * 1024 ? 2u : 1u;  // wavefronts per block
      const dim3 grid((P.item_cap + wpb - 1) / wpb, nb), block(64 * wpb);
      if (c->test_overlap) hipLaunchKernelGGL(k_test<true>, grid, block, lds_wave * wpb, sm, V, P.g0, P.g1, (uint32_t)j, P.item_off, P.item_cap, steps_cap);
      else hipLaunchKernelGGL(k_test<false>, grid, block, lds_wave * wpb, sm, V, P.g0, P.g1, (uint32_t)j, P.item_off, P.item_cap, steps_cap);
    }
  }
  if (part == 1) return;
  if (cfg.method == KS_METHOD_MERGED && cfg.enable_anti_grazing)
    hipLaunchKernelGGL(k_count_grazing<16>, dim3((uint32_t)((n + 15) / 16), nb), dim3(256), 0, sm, V);
  hipLaunchKernelGGL(k_scan_local, dim3((uint32_t)(((cfg.method == KS_METHOD_MERGED ? 2 : 1) * n + kScanBlock - 1) / kScanBlock), nb),
                     dim3(1024), 0, sm, V);
  launch_emit(c, V, nb, wide, sm);
  // the frames' only device->host traffic: pair / ray / tile counts and error flags
  hipLaunchKernelGGL(k_publish, dim3(nb), dim3(64), 0, sm, V, (const uint32_t*)c->table.n_tiles);
}

// fast, early-out in the reference's serial order: fix-point iteration over the rays' visited lengths, seeded by
// the ordered-phase result already in S.d_cnt (ks_k_exact.h).  Host waits inside: unpipelined contexts only.
int ensure_marks(ks_ctx* c, size_t n) {
  if (n <= c->cap_marks) return KS_OK;
  const size_t cap = std::max<size_t>(n + n / 4, 1 << 20);
  c->cap_marks = 0;
  int rc;
  for (int b = 0; b < 2; ++b) {
    if ((rc = c->d_eo_keys[b].alloc(c, cap))) return rc;
    if ((rc = c->d_eo_vals[b].alloc(c, cap))) return rc;
  }
  c->cap_marks = cap;
  return KS_OK;
}
constexpr int kEoMaxIterations = 4096;
int exact_early_out(ks_ctx* c, FrameSlot& S, hipStream_t st, Counters* counters = nullptr) {
  const size_t n = S.n;
  Counters* const d_counters = counters ? counters : S.d_counters;   // (the fallback of the event-driven path runs after k_publish has cleared the slot's own)
  const FrameParams* dF = S.d_F;
  EoState* hs = c->h_eo_state;
  HIPCHK(c, hipMemsetAsync(c->d_eo_state, 0, sizeof(EoState), st));
  hipLaunchKernelGGL(k_eo_total, dim3((uint32_t)std::min<size_t>((n + 255) / 256, 1024)), dim3(256), 0, st, dF,
                     (const uint32_t*)S.d_cnt, c->d_eo_state);
  HIPCHK(c, hipMemcpyAsync(hs, c->d_eo_state, sizeof(EoState), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const uint32_t nb4k = (uint32_t)((n + kScanBlock - 1) / kScanBlock);
  const size_t lds = (size_t)nb4k * sizeof(unsigned long long);
  uint64_t* kres = nullptr;
  uint32_t* vres = nullptr;
  unsigned long long n_marks = hs->n_marks_next;
  bool converged = n_marks == 0;
  int it = 0;
  for (; !converged && it < kEoMaxIterations; ++it) {
    int rc;
    if ((rc = ensure_marks(c, n_marks))) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_eo_range, 0, sizeof(uint2) << kSetBits, st));
    hipLaunchKernelGGL(k_eo_scan, dim3(nb4k), dim3(1024), 0, st, dF, (const uint32_t*)S.d_cnt, c->d_eo_lp, c->d_eo_bt, c->d_eo_state);
    if (S.wide)
      hipLaunchKernelGGL(k_eo_emit<8>, dim3((uint32_t)((n + 31) / 32)), dim3(256), lds, st, dF, S.d_ray_list, S.d_rays, S.d_cnt,
                         c->d_eo_lp, c->d_eo_bt, c->d_eo_keys[0], c->d_eo_vals[0], (unsigned long long)c->cap_marks, d_counters,
                         c->d_eo_state);
    else
      hipLaunchKernelGGL(k_eo_emit<64>, dim3((uint32_t)((n + 255) / 256)), dim3(256), lds, st, dF, S.d_ray_list, S.d_rays, S.d_cnt,
                         c->d_eo_lp, c->d_eo_bt, c->d_eo_keys[0], c->d_eo_vals[0], (unsigned long long)c->cap_marks, d_counters,
                         c->d_eo_state);
    // stable sort on the slot bits only: a slot's marks stay in (position, step) order
    // (as the fallback of the event-driven path this runs on the tail's thread and stream, beside stage A of later frames:
    // the tail's sort workspace, not stage A's)
    HIPCHK(c, (ksrs::sort<uint64_t, true>(counters ? c->sort_ws_tail : c->sort_ws, c->d_eo_keys[0], c->d_eo_keys[1], c->d_eo_vals[0], c->d_eo_vals[1],
                                          (size_t)n_marks, 64, st, &kres, &vres, 44)));
    hipLaunchKernelGGL(k_eo_index, dim3((uint32_t)((n_marks + 255) / 256)), dim3(256), 0, st, n_marks, (const uint64_t*)kres,
                       c->d_eo_range);
    EoBuf E{kres, vres, c->d_eo_range, c->d_eo_plain};
    if (S.wide)
      hipLaunchKernelGGL(k_eo_eval<8>, dim3((uint32_t)((n + 31) / 32)), dim3(256), 0, st, dF, S.d_ray_list, S.d_rays, S.d_cnt, E,
                         d_counters, c->d_eo_state);
    else
      hipLaunchKernelGGL(k_eo_eval<16>, dim3((uint32_t)((n + 63) / 64)), dim3(256), 0, st, dF, S.d_ray_list, S.d_rays, S.d_cnt, E,
                         d_counters, c->d_eo_state);
    HIPCHK(c, hipMemcpyAsync(hs, c->d_eo_state, sizeof(EoState), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (hs->n_marks != n_marks) {
      c->err = "exact early-out: mark count mismatch";
      return KS_ERR_HIP;
    }
    if (hs->changed == 0) converged = true;  // the marks just sorted are the frame's marks
    else n_marks = hs->n_marks_next;
  }
  if (!converged) {
    c->err = "exact early-out: no fixed point within the iteration limit";
    return KS_ERR_UNSUPPORTED;
  }
  c->eo_iterations += (uint64_t)it;
  if (!counters) c->eo_frames += 1;   // (as the fallback the frame has been counted)
  if (n_marks)
    hipLaunchKernelGGL(k_eo_commit, dim3((uint32_t)((n_marks + 255) / 256)), dim3(256), 0, st, n_marks, (const uint64_t*)kres,
                       (const uint32_t*)vres, c->d_eo_plain);
  return KS_OK;
}

// ---- exact early-out, event-driven (ks_k_exact.h) ----------------------------------------------------------------
// Per-slot buffers: the marks are sized from what earlier frames needed (a frame that does not fit falls back to the
// host-driven loop and asks for more: eo_want_*), everything else from the slot capacity.
int ensure_exact_slots(ks_ctx* c, size_t cap_marks, size_t cap_x) {
  if (!c->eo_device) return KS_OK;
  int rc;
  const int n_slots = c->cfg.pipeline_frames ? c->n_slots : 1;
  for (int i = 0; i < n_slots; ++i) {
    FrameSlot& S = c->slot[i];
    if (!S.d_eo_ctl) {
      if ((rc = S.d_eo_ctl.alloc(c, 1))) return rc;
      if ((rc = S.d_eo_tab.alloc(c, (size_t)1 << kSetBits))) return rc;
      HIPCHK(c, hipMemsetAsync(S.d_eo_tab, 0, sizeof(uint4) << kSetBits, c->stream));
      if ((rc = S.eo_committed.create(c, hipEventDisableTiming))) return rc;
    }
    if (S.eo_cap_marks < cap_marks) {
      S.eo_cap_marks = 0;
      for (int b = 0; b < 2; ++b) {
        if ((rc = S.d_eo_keys[b].alloc(c, cap_marks))) return rc;
        if ((rc = S.d_eo_vals[b].alloc(c, cap_marks))) return rc;
      }
      if ((rc = S.d_eo_sort_ws.alloc(c, ksrs::ws_words_dev(cap_marks, 3)))) return rc;
      if ((rc = S.d_eo_hitb.alloc(c, cap_marks))) return rc;
      if ((rc = S.d_eo_hseq.alloc(c, cap_marks))) return rc;
      if ((rc = S.d_eo_where.alloc(c, cap_marks))) return rc;
      if ((rc = S.d_eo_bits_a.alloc(c, cap_marks / 64 + 2))) return rc;
      if ((rc = S.d_eo_bits_b.alloc(c, cap_marks / 64 + 2))) return rc;
      S.eo_cap_marks = cap_marks;
    }
    if ((rc = S.d_eo_xnode.reserve(c, 2 * cap_x, 2 * cap_x))) return rc;
  }
  c->eo_cap_marks = cap_marks;
  c->eo_cap_x = cap_x;
  ++c->buffers_epoch;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KS_OK;
}
int ensure_exact_points(ks_ctx* c, size_t cap) {   // the per-position arrays (called by ensure_points)
  if (!c->eo_device) return KS_OK;
  int rc;
  for (int i = 0; i < (c->cfg.pipeline_frames ? c->n_slots : 1); ++i) {
    FrameSlot& S = c->slot[i];
    for (DevBuf<uint32_t>* p : {&S.d_eo_cnt_b, &S.d_eo_ux, &S.d_eo_dirty, &S.d_eo_list[0], &S.d_eo_list[1], &S.d_eo_chg, &S.d_eo_consulted, &S.d_eo_lp})
      if ((rc = p->alloc(c, cap))) return rc;
    if ((rc = S.d_eo_bt.alloc(c, cap / kScanBlock + 2))) return rc;
    if ((rc = S.d_eo_btp.alloc(c, cap / kScanBlock + 2))) return rc;
    if ((rc = S.d_eo_rinfo.alloc(c, cap))) return rc;
    if ((rc = S.d_eo_ckpt.alloc(c, 3 * cap))) return rc;
  }
  return KS_OK;
}
EoView eo_view(ks_ctx* c, const FrameSlot& S) {
  EoView E{};
  E.F = S.d_F;
  E.ray_list = S.d_ray_list;
  E.rays = S.d_rays;
  E.C = S.d_counters;
  E.cnt_a = S.d_cnt;
  E.cnt_b = S.d_eo_cnt_b;
  E.ux = S.d_eo_ux;
  E.dirty = S.d_eo_dirty;
  E.keys = S.d_eo_keys[1];   // three radix passes leave the sorted marks in the second buffer set
  E.vals = S.d_eo_vals[1];
  E.bits_a = S.d_eo_bits_a;
  E.bits_b = S.d_eo_bits_b;
  E.lp = S.d_eo_lp;
  E.bt = S.d_eo_bt;
  E.btp = S.d_eo_btp;
  E.keys0 = S.d_eo_keys[0];
  E.vals0 = S.d_eo_vals[0];
  E.cap_marks = (unsigned long long)S.eo_cap_marks;
  E.hitb = S.d_eo_hitb;
  E.hseq_w = S.d_eo_hseq;
  E.wide = S.wide ? 1u : 0u;
  E.live = S.d_live;
  E.hseq = S.d_eo_hseq;
  E.where = S.d_eo_where;
  E.rinfo = S.d_eo_rinfo;
  E.ckpt = S.d_eo_ckpt;
  E.tab = S.d_eo_tab;
  E.xnode = S.d_eo_xnode;
  E.cap_x = (uint32_t)(S.d_eo_xnode.size() / 2);
  E.list[0] = S.d_eo_list[0];
  E.list[1] = S.d_eo_list[1];
  E.chg = S.d_eo_chg;
  E.consulted = S.d_eo_consulted;
  E.plain = c->d_eo_plain;
  E.committed = c->d_eo_committed;
  E.ctl = S.d_eo_ctl;
  return E;
}
// long rays: `count` sweeps (each ends at once when the one before it changed nothing), ks_k_exact.h
void enqueue_sweeps(ks_ctx* c, const EoBatch& Bt, uint32_t nb, int count, hipStream_t st) {
  const size_t n = c->cap_points;
  const size_t waves = (size_t)order_chains_cap(c->cfg.integration_order_mode, n) *
                       ((order_generations_cap(c->cfg.integration_order_mode, n) + kEoSweepSegment - 1) / kEoSweepSegment);
  const uint32_t grid = (uint32_t)std::min<size_t>((waves + 3) / 4, 1 << 16);
  for (int i = 0; i < count; ++i) {
    hipLaunchKernelGGL(k_eo2_sweep, dim3(grid, nb), dim3(256), 0, st, Bt);
    hipLaunchKernelGGL(k_eo2_sweep_next, dim3(nb), dim3(64), 0, st, Bt);
  }
}
// part 1: the seeds' marks, sorted by slot, the full first iteration and the bulk rounds — for all nb frames of the batch
// per launch (after the ordered phases, which leave the seeds in the slots' d_cnt)
int enqueue_exact_rounds(ks_ctx* c, FrameSlot* const* slots, uint32_t nb, hipStream_t st) {
  const size_t n = c->cap_points;   // (grids by capacity: the kernels read the frame's own counts)
  const uint32_t nb4k = (uint32_t)((n + kScanBlock - 1) / kScanBlock);
  const size_t lds = (size_t)nb4k * sizeof(unsigned long long);
  EoBatch Bt{};
  ksrs::DevBatch<uint64_t> Rs{};
  const FrameSlot& S0 = *slots[0];
  for (uint32_t k = 0; k < nb; ++k) {
    const FrameSlot& S = *slots[k];
    Bt.v[k] = eo_view(c, S);
    Rs.keys_a[k] = S.d_eo_keys[0];
    Rs.keys_b[k] = S.d_eo_keys[1];
    Rs.vals_a[k] = S.d_eo_vals[0];
    Rs.vals_b[k] = S.d_eo_vals[1];
    Rs.n_dev[k] = (const unsigned long long*)&S.d_eo_ctl->st.n_marks;
    Rs.ws[k] = S.d_eo_sort_ws;
  }
  hipLaunchKernelGGL(k_eo2_begin, dim3(nb), dim3(64), 0, st, Bt);
  const uint32_t gm = (uint32_t)std::min<size_t>((S0.eo_cap_marks + 255) / 256, 2048);
  const uint32_t gn = (uint32_t)std::min<size_t>((n + 255) / 256, 2048);
  if (S0.wide) {
    // long rays: ONE emission whose views are the whole rays, then sweeps in integration order over the live bitmap, every
    // change applied at once (ks_k_exact.h); the sweeps end themselves when one of them changes nothing
    hipLaunchKernelGGL(k_eo2_full, dim3(gn, nb), dim3(256), 0, st, Bt);
    hipLaunchKernelGGL(k_eo2_scan, dim3(nb4k, nb), dim3(1024), 0, st, Bt);
    hipLaunchKernelGGL(k_eo2_emit<8>, dim3((uint32_t)((n + 31) / 32), nb), dim3(256), lds, st, Bt);
    HIPCHK(c, ksrs::sort_dev_batch<uint64_t>(Rs, (int)nb, S0.d_eo_sort_ws.size(), S0.eo_cap_marks, 44, 64, st));
    hipLaunchKernelGGL(k_eo2_bits, dim3(gm, nb), dim3(256), 0, st, Bt, 0u);
    hipLaunchKernelGGL(k_eo2_where, dim3(gm, nb), dim3(256), 0, st, Bt);
    enqueue_sweeps(c, Bt, nb, c->eo_sweeps, st);
    return KS_OK;
  } else {
    hipLaunchKernelGGL(k_eo2_scan, dim3(nb4k, nb), dim3(1024), 0, st, Bt);
    hipLaunchKernelGGL(k_eo2_emit<64>, dim3((uint32_t)((n + 255) / 256), nb), dim3(256), lds, st, Bt);
    // stable sort on the slot bits only: a slot's marks stay in (position, step) order; three passes: the result is in the
    // second buffer set (eo_view)
    HIPCHK(c, ksrs::sort_dev_batch<uint64_t>(Rs, (int)nb, S0.d_eo_sort_ws.size(), S0.eo_cap_marks, 44, 64, st));
    // the first iteration, full and streaming: hit bits of the sorted seed marks (and the slots' ranges), stop rule per ray,
    // validity bitmaps
    hipLaunchKernelGGL(k_eo2_hits, dim3(gm, nb), dim3(256), 0, st, Bt);
    hipLaunchKernelGGL(k_eo2_stop0, dim3(gn, nb), dim3(256), 0, st, Bt);
    hipLaunchKernelGGL(k_eo2_bits, dim3(gm, nb), dim3(256), 0, st, Bt, 1u);
  }
  // the event-driven rounds (round 0 was the full iteration above)
  // (wavefront per ray, grid-stride.  The lists shrink geometrically — ~3000 / 1000 / 600 / ... rays at 640x480 — and a
  // launch costs its workgroups: the later rounds get by with fewer, unless rays are long and lists stay long: 2 cm voxels)
  const uint32_t gr = (uint32_t)std::min<size_t>((n + 3) / 4, 2048);
  for (int r = 1; r <= c->eo_bulk_rounds; ++r) {
    const uint32_t g = S0.wide ? gr : std::min(gr, r == 1 ? 2048u : r == 2 ? 1024u : r <= 4 ? 512u : 256u);
    hipLaunchKernelGGL(k_eo2_eval, dim3(g, nb), dim3(256), 0, st, Bt, (uint32_t)r);
    hipLaunchKernelGGL(k_eo2_propagate, dim3(g, nb), dim3(256), 0, st, Bt, (uint32_t)r);
  }
  return KS_OK;
}
// part 2: what is left, by one workgroup, and the frame's marks into the shared table
void enqueue_exact_finish(ks_ctx* c, FrameSlot& S, hipStream_t st) {
  const EoView E = eo_view(c, S);
  hipLaunchKernelGGL(k_eo2_finish, dim3(1), dim3(kEoFinishThreads), 0, st, E, (uint32_t)c->eo_bulk_rounds + 1u, 1u);
  hipLaunchKernelGGL(k_eo2_commit, dim3(1024), dim3(256), 0, st, E);
}

// What `enqueue` puts on sm (it returns KS_OK, or the error that voids the capture), captured and instantiated; nullptr where
// the runtime refuses any of it.  Callers hold capture_mu.
template <typename Enqueue> hipGraphExec_t capture_graph(hipStream_t sm, Enqueue enqueue) {
  hipGraph_t g = nullptr;
  hipGraphExec_t out = nullptr;
  bool ok = hipStreamBeginCapture(sm, hipStreamCaptureModeRelaxed) == hipSuccess;
  if (ok) {
    const int rc = enqueue();
    ok = hipStreamEndCapture(sm, &g) == hipSuccess && g != nullptr && rc == KS_OK;
  }
  if (ok) ok = hipGraphInstantiate(&out, g, nullptr, nullptr, 0) == hipSuccess;
  if (g) (void)hipGraphDestroy(g);
  return ok ? out : nullptr;
}
// Stage B of one batch, in the three ways it is enqueued on the batch's march stream sm (launch_batch)
struct BatchLaunch {
  ks_ctx* c;
  FrameSlot* const* slots;
  uint32_t nb;
  FrameSlot& S0;             // the batch's first slot
  hipStream_t sm;
  const BatchView& V;
  size_t steps_max;
  uint64_t key;              // what the graphs in G have to be captured for
  FrameSlot::GraphSet& G;
  // long rays, plain launches: the sweeps go on until one of them changes nothing: the host reads two words per chunk of sweeps
  // (a frame is tens of milliseconds of GPU work here, and one frame at a time: ks_create)
  int sweeps_host_driven() const {
    EoBatch Bt{};
    for (uint32_t k = 0; k < nb; ++k) Bt.v[k] = eo_view(c, *slots[k]);
    for (int chunk = 1;; ++chunk) {
      bool going = false;
      for (uint32_t k = 0; k < nb; ++k) {
        uint32_t w[2] = {0u, 0u};   // {sw_prev, fail}
        HIPCHK(c, hipMemcpyAsync(&w[0], &slots[k]->d_eo_ctl->sw_prev, sizeof(uint32_t), hipMemcpyDeviceToHost, sm));
        HIPCHK(c, hipMemcpyAsync(&w[1], &slots[k]->d_eo_ctl->fail, sizeof(uint32_t), hipMemcpyDeviceToHost, sm));
        HIPCHK(c, hipStreamSynchronize(sm));
        going = going || (w[0] != 0u && w[1] == 0u);
      }
      if (!going || chunk >= c->eo_sweep_chunks) break;
      enqueue_sweeps(c, Bt, nb, c->eo_sweeps, sm);
    }
    hipLaunchKernelGGL(k_eo2_sweep_done, dim3(nb), dim3(64), 0, sm, Bt);
    return KS_OK;
  }
  // Exact early-out, event-driven (batches of one): the ordered phases give the seed; the event-driven fix point makes it the
  // serial result, on the device: three replayed graphs, the wait for the previous frame's marks between the first two
  int exact_device() const {
    int rc;
    auto seed_and_rounds = [&] {
      enqueue_stage_b(c, V, nb, S0.wide, sm, steps_max, 1);
      return enqueue_exact_rounds(c, slots, nb, sm);
    };
    auto finish = [&] {
      for (uint32_t k = 0; k < nb; ++k) enqueue_exact_finish(c, *slots[k], sm);   // (in frame order: a frame's finisher sees the marks of the one before)
      return KS_OK;
    };
    auto emission = [&] { return enqueue_stage_b(c, V, nb, S0.wide, sm, steps_max, 2), KS_OK; };
    bool graphs = c->use_graphs && !S0.wide;   // (long rays: the host looks at the sweeps' progress between chunks of them)
    if (graphs && (G.key != key || !G.g1 || !G.g2 || !G.g3)) {
      std::lock_guard<std::mutex> cap(c->capture_mu);
      G.reset();
      if ((G.g1 = capture_graph(sm, seed_and_rounds)) && (G.g2 = capture_graph(sm, finish)) && (G.g3 = capture_graph(sm, emission))) {
        G.key = key;
      } else {
        (void)hipGetLastError();
        G.reset();
        c->use_graphs = graphs = false;  // plain launches from now on
      }
    }
    if (graphs) HIPCHK(c, hipGraphLaunch(G.g1, sm));
    else if ((rc = seed_and_rounds()) || (S0.wide && (rc = sweeps_host_driven()))) return rc;
    if (c->eo_last_commit && c->eo_last_commit != S0.eo_committed) HIPCHK(c, hipStreamWaitEvent(sm, c->eo_last_commit, 0));
    if (graphs) HIPCHK(c, hipGraphLaunch(G.g2, sm));
    else finish();
    HIPCHK(c, hipEventRecord(S0.eo_committed, sm));   // (after the LAST frame's commit: the batch's frames finish in order on this stream)
    c->eo_last_commit = S0.eo_committed;
    if (graphs) HIPCHK(c, hipGraphLaunch(G.g3, sm));
    else emission();
    return KS_OK;
  }
  // Exact early-out, host-driven (batches of one): the ordered phases give the seed; the fix-point iteration (host waits inside) makes it serial
  int exact_host() const {
    enqueue_stage_b(c, V, nb, S0.wide, sm, steps_max, 1);
    if (int rc = exact_early_out(c, S0, sm)) return rc;
    enqueue_stage_b(c, V, nb, S0.wide, sm, steps_max, 2);
    return KS_OK;
  }
  // Every other mode: one sequence of launches, replayed from a graph unless the context does without or the runtime has refused a capture
  int plain_or_replayed() const {
    if (c->use_graphs && (G.key != key || !G.g1)) {
      std::lock_guard<std::mutex> cap(c->capture_mu);  // (rare: once per group of slots)
      G.reset();
      if ((G.g1 = capture_graph(sm, [&] { return enqueue_stage_b(c, V, nb, S0.wide, sm, steps_max), KS_OK; }))) {
        G.key = key;
      } else {
        (void)hipGetLastError();
        c->use_graphs = false;  // plain launches from now on
      }
    }
    if (c->use_graphs && G.g1) HIPCHK(c, hipGraphLaunch(G.g1, sm));
    else enqueue_stage_b(c, V, nb, S0.wide, sm, steps_max);
    return KS_OK;
  }
};

// Stage B of the frames whose stage A has been enqueued (consecutive frames, at most kBatchMax): ONE sequence of
// launches for all of them, captured once per (first slot, size) and replayed.  Called by the thread that enqueues
// stage A (graph capture and the helper thread's tail never meet on a stream).
int launch_batch(ks_ctx* c) {
  if (c->batch_slots.empty()) return KS_OK;
  std::vector<FrameSlot*> slots;
  slots.swap(c->batch_slots);
  const uint32_t nb = (uint32_t)slots.size();
  FrameSlot& S0 = *slots[0];
  hipStream_t sm = c->batch > 1 ? c->stream_march_[(S0.frame_no / (uint64_t)c->batch) % (uint64_t)c->n_march] : march_stream(c, S0.frame_no);
  c->prof_march_stream = sm;
  if (sm != c->stream) HIPCHK(c, hipStreamWaitEvent(sm, slots[nb - 1]->a_done, 0));  // stage A is one in-order stream: the last frame's event covers all
  const bool stage_events = nb == 1 && S0.prof_set >= 0 && c->pset[S0.prof_set].stages;
  if (stage_events) (void)hipEventRecord(c->pset[S0.prof_set].ev[4], sm);
  // The frames' parameters go to device memory; stage B's kernels take everything else from the slots, so
  // their launch sequence depends only on the capacity: it is captured once per group of slots and replayed.
  BatchView V{};
  size_t steps_max = 0;
  ParamsBatch PB{};
  for (uint32_t k = 0; k < nb; ++k) {
    FrameSlot& S = *slots[k];
    S.F.observed = observed_table(c, S.frame_no);
    if (c->exact_early_out) S.F.eo_frame = c->eo_frame_no++;
    if (S.F.frame_bits) S.F.frame_bits = (S.F.frame_bits & 0xffu) | (k << 8);
    S.batch_index = (int)k;
    S.batch_nb = (int)nb;
    for (uint32_t j = 0; j < (uint32_t)kBatchMax; ++j) S.batch_slots[j] = j < nb ? slots[j] : nullptr;
    S.tail_batched = false;
    PB.F[k] = S.F;
    PB.out[k] = S.d_F;
    V.s[k] = slot_view(S);
    steps_max = std::max(steps_max, S.steps_max);
  }
  if (nb == 1) hipLaunchKernelGGL(k_set_params, dim3(1), dim3(64), 0, sm, slots[0]->F, slots[0]->d_F);
  else hipLaunchKernelGGL(k_set_params_batch, dim3(nb), dim3(64), 0, sm, PB);   // (one launch at the head of the batch's chain instead of nb)
  const uint64_t key = ((uint64_t)c->cap_points << 24) ^ (c->buffers_epoch.load() << 4) ^ (S0.wide ? 1u : 0u) ^ ((uint64_t)nb << 1);
  const BatchLaunch B{c, slots.data(), nb, S0, sm, V, steps_max, key, S0.b_graphs[nb == (uint32_t)c->batch ? 0 : 1]};
  if (int rc = !c->exact_early_out ? B.plain_or_replayed() : c->eo_device && !c->eo_device_off ? B.exact_device() : B.exact_host()) return rc;
  for (uint32_t k = 0; k < nb; ++k) {
    HIPCHK(c, hipEventRecord(slots[k]->ready, sm));
    slots[k]->b_launched = true;
  }
  if (stage_events) (void)hipEventRecord(c->pset[S0.prof_set].ev[5], sm);
  return KS_OK;
}

// ---- front half: everything up to the counter snapshot --------------------------------------
// the frame's parameters from the context, the pose and the point count (stage A adds the order, the key window and the anti-grazing keys)
void fill_frame_params(ks_ctx* c, FrameParams& F, const float Tq[7], size_t n, int freespace) {
  const ks_config& cfg = c->cfg;
  F = FrameParams{};
  F.T.w = Tq[0];
  F.T.v = {Tq[1], Tq[2], Tq[3]};
  F.T.t = {Tq[4], Tq[5], Tq[6]};
  F.voxel_size_inv = c->voxel_size_inv;
  F.min_ray = cfg.min_ray_length_m;
  F.max_ray = cfg.max_ray_length_m;
  F.trunc = cfg.truncation_distance;
  F.start_inv = cfg.start_voxel_subsampling_factor * c->voxel_size_inv;
  F.log_match = c->log_match;
  F.log_non_match = c->log_non_match;
  F.tsdf.voxel_size = cfg.voxel_size;
  F.tsdf.trunc = cfg.truncation_distance;
  F.tsdf.max_weight = cfg.max_weight;
  F.tsdf.dropoff_denominator = cfg.truncation_distance - cfg.voxel_size;
  F.tsdf.sparsity_factor = cfg.sparsity_compensation_factor;
  F.tsdf.use_dropoff = cfg.use_weight_dropoff;
  F.tsdf.use_sparsity = cfg.use_sparsity_compensation_factor;
  F.start_offset = c->start_offset;
  F.observed_offset = c->observed_offset;
  F.obs_tag = c->obs_tag;
  F.obs_tag_lo = c->obs_tag_lo;
  F.max_collisions = cfg.max_consecutive_ray_collisions;
  F.n = (uint32_t)n;
  const uint32_t q = (uint32_t)(n / kOrderStep);
  const bool by_1024 = cfg.integration_order_mode == KS_ORDER_MIXED_1024_GROUPS;
  F.order_groups = q == 0 ? 1u : by_1024 ? kOrderStep : q;
  F.order_per = q == 0 ? 0u : by_1024 ? q : kOrderStep;
  F.chains = order_chains(cfg.integration_order_mode, n);
  F.carving = cfg.voxel_carving_enabled;
  F.allow_clear = cfg.allow_clear;
  F.freespace = freespace;
  F.use_const_weight = cfg.use_const_weight;
  F.method = cfg.method;
  F.color_mode = cfg.color_mode;
  F.sorted_order = cfg.integration_order_mode == KS_ORDER_SORTED;
  F.n_dynamic = cfg.n_dynamic_labels;
  const unsigned pb = bits_for(n);
  F.point_mask = (1u << pb) - 1u;
  F.clear_bit = (cfg.method == KS_METHOD_MERGED) ? (1u << pb) : 0u;
  F.seq_bits = pb + (cfg.method == KS_METHOD_MERGED ? 1u : 0u);
  if (const unsigned fb = tail_frame_bits(c)) {   // (point_mask stays the frame's own: key & point_mask is the ray sequence on every path)
    F.frame_bits = bits_for(c->cap_points);   // (the index joins it in launch_batch)
    F.seq_bits = F.frame_bits + fb;
  }
  F.inv_order = F.sorted_order ? c->d_inv_order : nullptr;
  std::memcpy(F.dynamic_labels, cfg.dynamic_labels, 32);
  // the early-out can never fire if the threshold exceeds the longest possible ray
  F.early_out = c->uses_early_out;
}
// the frame's profile set (its previous frame resolved first): which of its events this frame records
void begin_prof_set(ks_ctx* c, FrameSlot& S, size_t n) {
  const int set = (int)(c->frame_no % kProfSets);
  resolve_prof(c, set);
  ProfSet& P = c->pset[set];
  P.used = true;
  P.complete = P.applied = false;
  P.stages = c->profiling == 1;
  P.apply = c->profiling == 1 || (c->frame_no % 4) == 0;
  P.n_points = n;
  P.n_pairs = 0;
  S.prof_set = set;
}
// stage A of `fast`: rays per point, the start-voxel dedup by a stable sort on the slot, the seed's work list
int stage_a_fast(ks_ctx* c, FrameSlot& S, const float* d_xyz, const uint8_t* d_rgba, const uint8_t* d_labels, size_t n) {
  const FrameParams& F = S.F;
  hipStream_t st = c->stream;
  const uint32_t nb1k = (uint32_t)((n + 1023) / 1024);
  hipLaunchKernelGGL(k_points_fast, dim3(nb1k), dim3(1024), 0, st, F, d_xyz, d_rgba, d_labels, c->d_color_lut,
                     S.d_rays, c->d_hash, c->d_skeys32, c->d_pvals, S.d_cnt, S.d_live, S.d_counters);
  stage_mark(c, S.prof_set, 1);
  // stable sort by slot only: position order inside a slot is preserved
  uint32_t *sk = nullptr, *sv = nullptr;
  if (int rc = sort_pairs(c, c->d_skeys32.get(), c->d_skeys32b.get(), c->d_pvals.get(), c->d_pvals2.get(), n, kSetBits + 1, &sk, &sv)) return rc;
  stage_mark(c, S.prof_set, 2);
  hipLaunchKernelGGL(k_dedup, dim3(nb1k), dim3(1024), 0, st, F, sk, sv, c->d_hash, c->d_start_set, S.d_ray_list, S.d_rays, S.d_cnt, S.d_live, S.d_counters);
  if (c->uses_early_out && n > 0) {
    // live[] is final: the work list of the seed's phases (k_test), here and not at the head of stage B's chain of
    // dependent launches.  Only the phases this frame reaches.
    const uint32_t n_gen = (uint32_t)((n + F.chains - 1) / F.chains);
    uint32_t n_ph = 0;
    while (n_ph < c->seed_phases.size() && c->seed_phases[n_ph].g0 < n_gen) ++n_ph;
    HIPCHK(c, hipMemsetAsync(S.d_seed_n, 0, c->seed_phases.size() * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_seed_list, dim3((F.chains + 63u) / 64u, n_ph), dim3(64 * kSeedSegs), 0, st, F, (const SeedPhase*)c->d_seed_phases,
                       (const uint8_t*)S.d_live, S.d_seed_gen, S.d_seed_items, S.d_seed_n, S.d_counters);
  }
  hipLaunchKernelGGL(k_dedup_commit, dim3(nb1k), dim3(1024), 0, st, F, sk, sv, c->d_hash, c->d_start_set, S.d_counters);
  return KS_OK;
}
// the bundles' ranks in the iteration order of the reference's unordered_map (ks_k_bundle_order.h):
// insertion indices, then one walk + link launch per rehash epoch the slot capacity can reach
void enqueue_bundle_order(ks_ctx* c, hipStream_t st, size_t n, const uint64_t* sk, const uint32_t* sv) {
  const uint32_t capb = (uint32_t)((c->cap_points + kBoBlock - 1) / kBoBlock);
  const size_t lds_f = (2 * c->cap_points / kBoBlock + 3) * sizeof(uint32_t), lds_e = ((size_t)capb + 2) * sizeof(uint32_t);
  hipLaunchKernelGGL(k_bo_scan_flags, dim3((uint32_t)((2 * n + kBoBlock - 1) / kBoBlock)), dim3(kBoBlock), 0, st, (uint32_t)n, c->bo);
  hipLaunchKernelGGL(k_bo_init, dim3((uint32_t)((n + kBoBlock - 1) / kBoBlock)), dim3(kBoBlock), lds_f, st, (uint32_t)n, sk, sv, c->bo);
  const uint32_t nbb = (uint32_t)((n + kBoBlock - 1) / kBoBlock);  // a frame of n points has at most n bundles
  // epochs whose bucket count fits one workgroup's LDS: one launch for all of them (both maps)
  int e_small = 0;
  while (e_small < c->bo_epochs && c->bo_sched.b[e_small] <= kBoSmallBuckets) ++e_small;
  if (e_small > 0) hipLaunchKernelGGL(k_bo_small, dim3(2), dim3(kBoBlock), 0, st, c->bo, e_small);
  // (at least the first launch pair's k_bo_link goes out: it takes over from k_bo_small)
  const size_t nh_floor = c->bo_hint_fixed ? (e_small > 0 ? (size_t)c->bo_sched.t[e_small - 1] + 1 : 1) : 2 * (size_t)kBoSmallBuckets;
  const size_t nh = std::min<size_t>(n, std::max<size_t>(c->bo_hint.load(std::memory_order_relaxed), nh_floor));
  int e_last = -1;   // the epoch whose k_bo_link went out without its k_bo_walk
  for (int e = e_small; e <= c->bo_epochs; ++e) {
    if (e > 0 && c->bo_sched.t[e - 1] >= nh) break;  // no map of nh bundles reaches epoch e - 1
    hipLaunchKernelGGL(k_bo_link, dim3(nbb, 2), dim3(kBoBlock), lds_e, st, c->bo, e, (e == e_small && e_small > 0) ? 1 : 0);
    if (e < c->bo_epochs && c->bo_sched.t[e] < nh)
      hipLaunchKernelGGL(k_bo_walk, dim3(nbb, 2), dim3(kBoBlock), 0, st, c->bo, e);
    else
      e_last = e;
  }
  // (a map with more bundles than the hint: the rest of the recurrence, one workgroup per map)
  if (nh < n && e_last >= 0 && e_last < c->bo_epochs) hipLaunchKernelGGL(k_bo_rest, dim3(2), dim3(kBoBlock), lds_e, st, c->bo, e_last);
}
// stage A of `merged`: end-voxel keys per point, sorted; the points gathered in that order; bundles of points per end voxel
int stage_a_merged(ks_ctx* c, FrameSlot& S, const float* d_xyz, const uint8_t* d_rgba, const uint8_t* d_labels, size_t n, const uint32_t* order_ptr) {
  const ks_config& cfg = c->cfg;
  FrameParams& F = S.F;
  hipStream_t st = c->stream;
  const uint32_t nb = (uint32_t)((n + 255) / 256);
  const uint32_t nb1k = (uint32_t)((n + 1023) / 1024);
  if (c->key_bits) {
    // the key window of this frame: every point within max_ray of the sensor (all but far clearing points) is inside
    const float reach = cfg.max_ray_length_m + 2.0f * cfg.voxel_size;
    const float tq[3] = {F.T.t.x, F.T.t.y, F.T.t.z};
    for (int a = 0; a < 3; ++a) {
      const float lo = std::floor((tq[a] - reach) * c->voxel_size_inv) - 2.0f;
      F.key_base[a] = (int32_t)std::min(std::max(lo, -2.0e9f), 2.0e9f);
    }
    F.key_bits = c->key_bits;
  }
  hipLaunchKernelGGL(k_points_merged, dim3(nb1k), dim3(1024), 0, st, F, d_xyz, d_rgba, d_labels, c->d_color_lut, c->d_pkeys, c->d_skeys32, c->d_pvals,
                     S.d_cnt, c->use_bundle_rank ? c->bo.flag : nullptr, c->d_key_overflow, c->key_overflow_mask, S.d_counters);
  stage_mark(c, S.prof_set, 1);
  uint64_t* sk = nullptr;
  uint32_t *sk32 = nullptr, *sv = nullptr;
  if (c->key_bits) {
    // four passes over 32-bit grouping keys instead of eight over the 64-bit end-voxel keys; k_gather_sorted writes the
    // sorted 64-bit keys for everything downstream
    if (int rc = sort_pairs(c, c->d_skeys32.get(), c->d_skeys32b.get(), c->d_pvals.get(), c->d_pvals2.get(), n, 32, &sk32, &sv)) return rc;
    sk = c->d_pkeys;
  } else {
    if (int rc = sort_pairs(c, c->d_pkeys.get(), c->d_pkeys2.get(), c->d_pvals.get(), c->d_pvals2.get(), n, 64, &sk, &sv)) return rc;
  }
  stage_mark(c, S.prof_set, 2);
  hipLaunchKernelGGL(k_gather_sorted, dim3(nb), dim3(256), 0, st, F, d_xyz, d_rgba, d_labels, c->d_color_lut,
                     order_ptr, (const uint64_t*)sk, (const uint32_t*)sk32, sk, sv, c->d_gpw, c->d_glc, c->use_bundle_rank ? c->bo.flag : nullptr, c->d_blong,
                     c->d_key_overflow, S.d_counters);
  if (c->use_bundle_rank) enqueue_bundle_order(c, st, n, sk, sv);
  // anti-grazing: the frame keeps its own copy of the keys (the next frame's stage A reuses the sort
  // buffers while this frame's emission — or its repetition after a pair-buffer overflow — may still run)
  uint64_t* ray_keys = cfg.enable_anti_grazing ? S.d_rkeys : nullptr;
  if (cfg.enable_anti_grazing) HIPCHK(c, hipMemcpyAsync(S.d_gkeys, sk, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  // one launch: the bundles of kLongRun points and more (one serial chain per bundle, 0.16 ms at 640x480 with a wall close
  // to the sensor) in the first workgroups, the short bundles under them
  const uint32_t n_long_blocks = (uint32_t)std::min<size_t>(n / kLongRun + 1, 512);
  hipLaunchKernelGGL(k_bundles_all, dim3(n_long_blocks + (uint32_t)((n + 127) / 128)), dim3(128), 0, st, F, sk, sv, c->d_gpw, c->d_glc, c->d_blong,
                     S.d_rays, S.d_deltas, S.d_ray_list, ray_keys, S.d_cnt, c->bo, c->use_bundle_rank, S.d_counters, n_long_blocks);
  if (cfg.enable_anti_grazing) {
    F.grazing_keys = S.d_gkeys;
    F.ray_keys = S.d_rkeys;
  }
  return KS_OK;
}
int frame_front(ks_ctx* c, FrameSlot& S, const float Tq[7], const float* d_xyz, const uint8_t* d_rgba, const uint8_t* d_labels, size_t n, int freespace) {
  int rc;
  FrameParams& F = S.F;
  fill_frame_params(c, F, Tq, n, freespace);
  // longest possible ray in steps: long rays get a whole wavefront per ray in stage B, short ones 16 lanes
  const size_t steps_max = steps_max_of(c->cfg, c->voxel_size_inv);
  S.wide = steps_max > 400;
  const size_t hint = c->pairs_hint.load(std::memory_order_relaxed);
  if ((rc = ensure_pairs_in(c, S, std::max<size_t>(hint + hint / 4, 1 << 20)))) return rc;
  hipStream_t st = c->stream;
  if (S.tail_recorded && c->stream_tail != c->stream) HIPCHK(c, hipStreamWaitEvent(st, S.tail_done, 0));
  if (S.join_recorded) HIPCHK(c, hipStreamWaitEvent(st, S.join, 0));  // (its long runs may have ended after its tail_done)
  S.n = n;
  S.prof_set = -1;
  if (c->profiling) begin_prof_set(c, S, n);
  S.frame_no = c->frame_no++;
  // S.d_counters are zero: cleared at create time / by k_publish of the slot's previous frame
  const uint32_t nb = (uint32_t)((n + 255) / 256);
  const uint32_t* order_ptr = nullptr;
  stage_mark(c, S.prof_set, 0);
  if (F.sorted_order) {
    hipLaunchKernelGGL(k_sqnorm, dim3(nb), dim3(256), 0, st, (uint32_t)n, d_xyz, c->d_okeys, c->d_ovals);
    uint32_t *ok = nullptr, *ov = nullptr;
    if ((rc = sort_pairs(c, c->d_okeys.get(), c->d_okeys2.get(), c->d_ovals.get(), c->d_order.get(), n, 32, &ok, &ov))) return rc;
    order_ptr = ov;  // position -> index
    hipLaunchKernelGGL(k_invert, dim3(nb), dim3(256), 0, st, (uint32_t)n, order_ptr, c->d_inv_order);
    F.order = order_ptr;
  }
  if ((rc = c->cfg.method == KS_METHOD_FAST ? stage_a_fast(c, S, d_xyz, d_rgba, d_labels, n) : stage_a_merged(c, S, d_xyz, d_rgba, d_labels, n, order_ptr)))
    return rc;
  stage_mark(c, S.prof_set, 3);
  // ---- stage B (early-out phases, scan, pair emission) is enqueued per BATCH of frames: launch_batch
  if (c->stream_march_[0] != st) HIPCHK(c, hipEventRecord(S.a_done, st));
  S.steps_max = steps_max;
  S.b_launched = false;
  S.pending = true;
  c->batch_slots.push_back(&S);
  if ((int)c->batch_slots.size() >= c->batch || c->profiling == 1) return launch_batch(c);
  return KS_OK;
}

// ---- tail half: sized by the snapshot --------------------------------------------------------
// Marcher: records of the frame in S (ks_k_shard.h), stable-partitioned by owner into d_sh_*[1]; counts on the host.
int shard_export_frame(ks_ctx* c, FrameSlot& S, unsigned long long n_pairs, hipStream_t st) {
  const int world = c->shard_world;
  int rc;
  if (n_pairs > c->cap_sh) {
    const size_t cap = std::max<size_t>(n_pairs + n_pairs / 4, 1 << 20);
    c->cap_sh = 0;
    for (int b = 0; b < 2; ++b) {
      if ((rc = c->d_sh_okey[b].alloc(c, cap))) return rc;
      if ((rc = c->d_sh_gkey[b].alloc(c, cap))) return rc;
      if ((rc = c->d_sh_seq[b].alloc(c, cap))) return rc;
      if ((rc = c->d_sh_sdf[b].alloc(c, cap))) return rc;
      if ((rc = c->d_sh_uw[b].alloc(c, cap))) return rc;
    }
    c->cap_sh = cap;
  }
  if (!c->d_sh_counts && (rc = c->d_sh_counts.alloc(c, 128))) return rc;
  const bool merged = c->cfg.method == KS_METHOD_MERGED;
  c->shm_counts[0] = c->shm_counts[1] = 0;
  if (merged && (S.n > c->cap_shm_n || !c->d_shm_cnt)) {
    const size_t cap = std::max<size_t>(S.n, 1 << 16);
    c->cap_shm_n = 0;
    if ((rc = c->d_shm_bno.alloc(c, cap))) return rc;
    if ((rc = c->d_shm_btab.alloc(c, cap))) return rc;
    if ((rc = c->d_shm_mpos.alloc(c, cap))) return rc;
    if ((rc = c->d_shm_cnt.alloc(c, 2))) return rc;
    c->cap_shm_n = cap;
  }
  HIPCHK(c, hipMemsetAsync(c->d_sh_counts, 0, 128 * sizeof(uint32_t), st));
  std::memset(c->sh_counts, 0, sizeof(c->sh_counts));
  c->sh_exported = n_pairs;
  if (n_pairs) {
    const uint32_t nb = (uint32_t)((n_pairs + 255) / 256);
    hipLaunchKernelGGL(k_shard_export, dim3(nb), dim3(256), 0, st, S.F, n_pairs, (const uint64_t*)S.d_pairs, (const RayDesc*)S.d_rays,
                       (const uint64_t*)c->table.slot_keys, (uint32_t)world, c->d_sh_okey[0], c->d_sh_gkey[0], c->d_sh_seq[0],
                       c->d_sh_sdf[0], c->d_sh_uw[0], c->d_sh_counts);
    uint64_t* sorted = nullptr;
    HIPCHK(c, (ksrs::sort<uint64_t, false>(c->sort_ws_tail, c->d_sh_okey[0], c->d_sh_okey[1], nullptr, nullptr, (size_t)n_pairs, 64, st,
                                           &sorted, nullptr, 56)));
    if (merged) {
      // the bundles that have an update are numbered; the records name the number, the two tables carry the increments
      HIPCHK(c, hipMemsetAsync(c->d_shm_bno, 0, (size_t)S.n * sizeof(uint32_t), st));
      HIPCHK(c, hipMemsetAsync(c->d_shm_cnt, 0, 2 * sizeof(uint32_t), st));
      hipLaunchKernelGGL(k_shard_mark_bundles, dim3(nb), dim3(256), 0, st, n_pairs, (const uint32_t*)c->d_sh_seq[0], c->d_shm_bno);
      hipLaunchKernelGGL(k_shard_bundle_table, dim3((uint32_t)((S.n + 255) / 256)), dim3(256), 0, st, (uint32_t)S.n, (const RayDesc*)S.d_rays,
                         c->d_shm_bno, c->d_shm_btab, c->d_shm_mpos, c->d_shm_cnt);
      hipLaunchKernelGGL(k_shard_gather_merged, dim3(nb), dim3(256), 0, st, n_pairs, (const uint64_t*)sorted, (const uint64_t*)c->d_sh_gkey[0],
                         (const uint32_t*)c->d_sh_seq[0], (const float*)c->d_sh_sdf[0], (const float*)c->d_sh_uw[0], (const uint32_t*)c->d_shm_bno,
                         c->d_sh_gkey[1], c->d_sh_seq[1], c->d_sh_sdf[1], c->d_sh_uw[1]);
      HIPCHK(c, hipMemcpyAsync(c->shm_counts, c->d_shm_cnt, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    } else {
      hipLaunchKernelGGL(k_shard_gather, dim3(nb), dim3(256), 0, st, n_pairs, (const uint64_t*)sorted, (const uint64_t*)c->d_sh_gkey[0],
                         (const uint32_t*)c->d_sh_seq[0], (const float*)c->d_sh_sdf[0], (const float*)c->d_sh_uw[0], c->d_sh_gkey[1],
                         c->d_sh_seq[1], c->d_sh_sdf[1], c->d_sh_uw[1]);
    }
    HIPCHK(c, hipMemcpyAsync(c->sh_counts, c->d_sh_counts, 65 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  if (merged && c->shm_counts[1]) {
    const size_t nm = c->shm_counts[1];
    if ((rc = c->d_shm_mixed.reserve(c, nm * kNumLabels, std::max<size_t>(nm + nm / 2, 1024) * kNumLabels))) return rc;
    hipLaunchKernelGGL(k_shard_mixed_rows, dim3((uint32_t)((nm * kNumLabels + 255) / 256)), dim3(256), 0, st, (uint32_t)nm,
                       (const uint32_t*)c->d_shm_mpos, (const float*)S.d_deltas, c->d_shm_mixed);
    HIPCHK(c, hipStreamSynchronize(st));
  }
  return KS_OK;
}

// the update's stage events of a frame that does not reach the update (an error, a marcher's export, no pairs)
inline void skip_update_stages(ks_ctx* c, int set) {
  for (int e = 7; e < kStageEvents - 1; ++e) stage_mark(c, set, e);
}
// the last event of the frame's profile set: the set is complete
inline void finish_prof(ks_ctx* c, int set, hipStream_t st, uint64_t n_pairs) {
  if (set < 0) return;
  ProfSet& P = c->pset[set];
  P.n_pairs = n_pairs;
  (void)hipEventRecord(P.ev[kStageEvents - 1], st);
  P.complete = true;
}
// the frame's statistics, owed to the caller until the next hand-over (deliver_stats)
inline void owe_stats(ks_ctx* c, const FrameSlot& S, const Counters& cnt, unsigned long long n_pairs, uint32_t n_blocks) {
  c->owed.n_points += S.n;
  c->owed.n_valid_points += cnt.n_valid;
  c->owed.n_rays_cast += cnt.n_rays;
  c->owed.n_voxel_updates += n_pairs;
  c->owed.n_blocks_allocated += n_blocks;
}
// How the early-out buffers are to grow after a fallback (hctl: the frame's control block as the device left it): requests only, nothing is launched
void eo_grow_after_fallback(ks_ctx* c, const EoCtl& hctl) {
  // (the largest request of the frames that failed since the buffers last grew: a later frame's smaller one must not replace it)
  auto want_at_least = [](auto& w, auto v) {
    auto cur = w.load(std::memory_order_relaxed);
    while (cur < v && !w.compare_exchange_weak(cur, v, std::memory_order_relaxed)) {}
  };
  if (hctl.fail & kEoFailMarks) want_at_least(c->eo_want_marks, std::max<size_t>(2 * c->eo_cap_marks, (size_t)hctl.st.n_marks + (size_t)hctl.st.n_marks / 4));
  // X marks are for the few rays the seed stopped too early; a frame that wants more of them than an eighth of its
  // marks (2 cm voxels / 10 m rays: the approximate set is overwhelmed, the seed is wrong on most rays) is not a sparse
  // problem, and neither is one whose lists are still long after the bulk rounds
  const bool x_dense = (hctl.fail & kEoFailX) && (size_t)hctl.n_x > (size_t)hctl.st.n_marks / 8;
  // lists still long when the finisher takes over: more rounds as launches for the frames to come, while there is room
  const bool more_bulk = (hctl.fail & kEoFailRounds) && !x_dense && c->eo_bulk_rounds < (int)kEoBulkMax;
  if (more_bulk) want_at_least(c->eo_want_bulk, std::min((int)kEoBulkMax, c->eo_bulk_rounds + std::max(4, c->eo_bulk_rounds / 2)));
  const bool dense = x_dense || ((hctl.fail & kEoFailRounds) && !more_bulk);
  // (the count at the moment of the failure is a lower bound — the rounds stop there — and every growth costs the frames in
  // flight a repetition on the host: grow generously, a node is 16 bytes)
  if ((hctl.fail & kEoFailX) && !dense) want_at_least(c->eo_want_x, std::max<size_t>(16 * c->eo_cap_x, 8 * (size_t)hctl.n_x));
  if (dense) c->eo_hopeless.fetch_add(1, std::memory_order_relaxed);
  else if (!(hctl.fail & kEoFailChain)) c->eo_hopeless.store(0, std::memory_order_relaxed);
}
// The frame's emission once more, on the tail stream, counted in d_retry_counters (k_publish has cleared the slot's counters); the host
// waits for it.  fix_point_first: the host-driven fix point, the frame's mark in the shared table and k_scan_local go in front (after a
// fallback the slot holds no scan).  Leaves the repetition's err and n_pairs in *cnt and the table's tile count in *new_tiles.
int repeat_emission(ks_ctx* c, FrameSlot& S, hipStream_t st, bool fix_point_first, Counters* cnt, uint32_t* new_tiles) {
  Counters rcnt{};
  rcnt.n_rays = cnt->n_rays;
  HIPCHK(c, hipMemcpyAsync(c->d_retry_counters, &rcnt, sizeof(rcnt), hipMemcpyHostToDevice, st));
  BatchView V{};
  V.s[0] = slot_view(S, c->d_retry_counters);
  if (fix_point_first) {
    if (int rc = exact_early_out(c, S, st, c->d_retry_counters)) return rc;
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)c->d_eo_committed, (int)(S.F.eo_frame + 1u), 1, st));
    hipLaunchKernelGGL(k_scan_local, dim3((uint32_t)((c->cap_points + kScanBlock - 1) / kScanBlock), 1), dim3(1024), 0, st, V);
  }
  launch_emit(c, V, 1, S.wide, st);
  HIPCHK(c, hipMemcpyAsync(&rcnt, c->d_retry_counters, sizeof(rcnt), hipMemcpyDeviceToHost, st));
  uint32_t nt = 0;
  HIPCHK(c, hipMemcpyAsync(&nt, c->table.n_tiles, sizeof(nt), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  cnt->err = rcnt.err;
  cnt->n_pairs = rcnt.n_pairs;
  *new_tiles = std::min(nt, c->cfg.max_tiles);
  return KS_OK;
}
// The device-driven fix point gave up (marks or X marks did not fit, the finisher ran out of rounds, or the frame
// before this one fell back and had not entered its marks yet): the host-driven loop repeats the fix point from
// whatever lengths the slot holds (any seed converges), enters the marks, and scan + emission run again — as after a
// pair-buffer overflow, on the tail stream only.  Nothing was emitted and no tile was allocated by this frame.
int repair_after_fallback(ks_ctx* c, FrameSlot& S, hipStream_t st, Counters* cnt, uint32_t* new_tiles) {
  HIPCHK(c, hipStreamSynchronize(st));
  EoCtl hctl;
  HIPCHK(c, hipMemcpy(&hctl, S.d_eo_ctl, sizeof(hctl), hipMemcpyDeviceToHost));
  eo_grow_after_fallback(c, hctl);
  c->eo_fallbacks.fetch_add(1, std::memory_order_relaxed);
  return repeat_emission(c, S, st, /*fix_point_first=*/true, cnt, new_tiles);
}
// The frame's pairs did not fit the buffer sized from earlier frames: nothing was written and no tile was allocated.  Grow it and
// repeat the emission (the scan of the counts is still in the slot).  Later frames may already have allocated tiles; the emission
// is a get-or-insert, so that is harmless.
// (This runs on the helper thread while the caller may be capturing stage B of another slot on a march stream: nothing here may touch
// a march stream.  None has to: S.ready has ordered this slot's stage B, the tail stream is this thread's own, and no other frame
// reads this slot's pair buffer.)
int repair_after_overflow(ks_ctx* c, FrameSlot& S, hipStream_t st, Counters* cnt, uint32_t* new_tiles) {
  HIPCHK(c, hipStreamSynchronize(st));
  if (int rc = ensure_pairs_in(c, S, (size_t)cnt->n_pairs + (size_t)cnt->n_pairs / 4)) return rc;
  return repeat_emission(c, S, st, /*fix_point_first=*/false, cnt, new_tiles);
}
// the frame's error bits as the caller's error (the profile set is closed first)
int take_error_exits(ks_ctx* c, int set, hipStream_t st, uint32_t err) {
  skip_update_stages(c, set);
  finish_prof(c, set, st, 0);
  if (err & kErrLabel) {
    c->err = "semantic label >= 21 (CHECK_LT in the reference)";
    return KS_ERR_LABEL_RANGE;
  }
  c->fatal = true;
  c->err = (err & kErrPool) ? "voxel tile pool exhausted: raise ks_config.max_tiles" : "voxel index out of the packed range / tile table full";
  return (err & kErrPool) ? KS_ERR_POOL_FULL : KS_ERR_INDEX_RANGE;
}
// ---- the voxel update: k_apply / k_apply_runs on the tail stream, the long and xlong runs beside it ----------------------
// one launch: timed by its own begin / end events, or plain (a macro: the functional model reports a launch by the kernel's name as written)
#define KS_LAUNCH_TIMED_IF(timed, ev0, ev1, kernel, grid, block, stream, ...)                 \
  if (timed) hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, ev0, ev1, 0, __VA_ARGS__); \
  else hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__)
// what the update kernels of one frame are launched with, and their launches by colour mode and method
struct UpdateLaunch {
  ks_ctx* c;
  const FrameSlot& S;
  const FrameParams& F;
  hipStream_t st, sl, sx;   // tail | long runs | xlong runs (null: the context has no xlong kernel)
  int set, par;             // profile set (-1: none) | parity buffer set
  uint64_t* sp;             // the sorted pairs
  unsigned long long n_pairs, *d_long_list, *d_xlong_list;
  bool by_runs, time_apply, lanes_on;
  template <int MODE, bool MERGED> void apply() const {
    if (by_runs) {
      // k_apply_runs: 256 threads (tiles of 1024 pairs), not 512 (tiles of 2048).  Measured at 1280x720 / 2 cm beside the long-run
      // kernels: 2.45 vs 3.08 ms, the frame 5.98 vs 6.26 ms (profiles/r06_c4_merged_ab.txt) — a workgroup of one wavefront per SIMD
      // finds room where one of two per SIMD does not
      const uint32_t rb = (uint32_t)((n_pairs + kRunPer * 256u - 1) / (kRunPer * 256u));
      KS_LAUNCH_TIMED_IF(time_apply, c->pset[set].k0, c->pset[set].k1, (k_apply_runs<MODE, MERGED, 256u>), dim3(rb), dim3(256), st, F, n_pairs, sp,
                         S.d_rays.get(), S.d_deltas.get(), c->table, c->pool, c->d_label_lut.get(), kLongRun);
    } else {
      const uint32_t ab = (uint32_t)((n_pairs + 255) / 256);
      KS_LAUNCH_TIMED_IF(time_apply, c->pset[set].k0, c->pset[set].k1, (k_apply<MODE, MERGED>), dim3(ab), dim3(256), st, F, n_pairs, sp,
                         S.d_rays.get(), S.d_deltas.get(), c->table, c->pool, c->d_label_lut.get(), d_long_list, S.d_counters);
    }
  }
  template <int MODE> void xlong_runs() const {
    const uint32_t xb = (uint32_t)std::min<unsigned long long>(n_pairs / kXLongRun + 1, 512);
    if (c->xl_parallel && n_pairs >= c->xl_min_pairs) {
      // the class sums and the weight of such runs as integer sums per chunk, chunks side by side (ks_k_apply_xl.h); what
      // the shortcut cannot carry goes to k_apply_xlong through the fall-back list
      hipLaunchKernelGGL(k_xl_measure<MODE>, dim3(kXlMaxRuns / 256), dim3(256), 0, sx, F, n_pairs, (const uint64_t*)sp, c->pool,
                         (const unsigned long long*)d_xlong_list, (const Counters*)S.d_counters, c->d_xl_runs);
      hipLaunchKernelGGL(k_xl_number, dim3(1), dim3(1024), 0, sx, (const unsigned long long*)d_xlong_list, (const Counters*)S.d_counters,
                         c->d_xl_runs, c->d_xl_idx, c->d_xl_fb, c->d_xl_hdr, c->cap_xl_chunks);
      hipLaunchKernelGGL(k_xl_chunks, dim3(4096), dim3(256), 0, sx, F, (const uint64_t*)sp, (const RayDesc*)S.d_rays, (const float*)S.d_deltas,
                         c->table, c->d_xl_runs, (const uint32_t*)c->d_xl_idx, (const XlHeader*)c->d_xl_hdr, c->d_xl_chunks);
      hipLaunchKernelGGL(k_xl_walk<MODE>, dim3(2048), dim3(64), 0, sx, F, (const uint64_t*)sp, (const RayDesc*)S.d_rays, (const float*)S.d_deltas,
                         c->table, c->pool, (const uint32_t*)c->d_label_lut, c->d_xl_runs, (const uint32_t*)c->d_xl_idx, c->d_xl_hdr,
                         (const XlChunk*)c->d_xl_chunks, c->d_xl_fb);
      hipLaunchKernelGGL(k_apply_xlong<MODE>, dim3(xb), dim3(256), 0, sx, F, n_pairs, sp, S.d_rays, S.d_deltas, c->table, c->pool, c->d_label_lut,
                         (const unsigned long long*)c->d_xl_fb, (const uint32_t*)&c->d_xl_hdr->n_fallback);
    } else {
      hipLaunchKernelGGL(k_apply_xlong<MODE>, dim3(xb), dim3(256), 0, sx, F, n_pairs, sp, S.d_rays, S.d_deltas, c->table, c->pool, c->d_label_lut,
                         d_xlong_list, (const uint32_t*)&S.d_counters->n_xlong);
    }
  }
  // the runs of kLongRun updates and more, a wavefront per run; with lanes_on, bucketed by length, a lane per run first
  template <int MODE> void long_runs() const {
    const uint32_t lb = (uint32_t)std::min<unsigned long long>(n_pairs / kLongRun + 1, 4096);
    if (lanes_on) {
      const uint32_t cap_long = (uint32_t)(n_pairs / (kLongRun + 1) + 1);
      hipLaunchKernelGGL(k_long_measure, dim3((cap_long + 255) / 256), dim3(256), 0, sl, F.seq_bits, n_pairs, (const uint64_t*)sp, d_long_list,
                         (const Counters*)S.d_counters, c->d_long_hdr_[par], kLongRun);
      hipLaunchKernelGGL(k_long_bucket, dim3((cap_long + 255) / 256), dim3(256), 0, sl, (const unsigned long long*)d_long_list,
                         (const Counters*)S.d_counters, c->d_long_hdr_[par], c->d_long_sorted_[par]);
      hipLaunchKernelGGL((k_apply_long_lanes<MODE, 6u>), dim3((cap_long / 64 + kLongClasses + 3) / 4), dim3(256), 0, sl, F, (const uint64_t*)sp,
                         (const RayDesc*)S.d_rays, (const float*)S.d_deltas, c->table, c->pool, (const uint32_t*)c->d_label_lut,
                         (const LongHdr*)c->d_long_hdr_[par], (const unsigned long long*)c->d_long_sorted_[par]);
      hipLaunchKernelGGL(k_apply_long<MODE>, dim3(std::min<uint32_t>(lb, 1024u)), dim3(128), 0, sl, F, n_pairs, sp, S.d_rays, S.d_deltas, c->table,
                         c->pool, c->d_label_lut, (const unsigned long long*)c->d_long_sorted_[par], (const Counters*)S.d_counters,
                         (const LongHdr*)c->d_long_hdr_[par]);
    } else {
      hipLaunchKernelGGL(k_apply_long<MODE>, dim3(lb), dim3(128), 0, sl, F, n_pairs, sp, S.d_rays, S.d_deltas, c->table, c->pool, c->d_label_lut,
                         d_long_list, S.d_counters);
    }
  }
  template <int MODE> void launch() const {
    c->cfg.method == KS_METHOD_MERGED ? apply<MODE, true>() : apply<MODE, false>();
    stage_mark(c, set, 9);
    if (sx) xlong_runs<MODE>();
    long_runs<MODE>();
  }
};
// ... of a whole batch of `fast` frames: the short runs, the xlong runs, the long runs (what differs between the frames comes from `tab`)
struct BatchUpdateLaunch {
  ks_ctx* c;
  const FrameParams& F;
  hipStream_t st, sl, sx;
  int set;                  // the profile set whose k0 / k1 time k_apply_batch (-1: none)
  uint64_t* sp;
  unsigned long long n_pairs, *d_long_list, *d_xlong_list;
  const TailFrame* tab;
  Counters* C;
  template <int MODE> void launch() const {
    const uint32_t ab = (uint32_t)((n_pairs + 255) / 256);
    KS_LAUNCH_TIMED_IF(set >= 0, c->pset[set].k0, c->pset[set].k1, (k_apply_batch<MODE>), dim3(ab), dim3(256), st, F, n_pairs, (const uint64_t*)sp, tab,
                       c->table, c->pool, (const uint32_t*)c->d_label_lut.get());
    if (sx) {
      const uint32_t xb = (uint32_t)std::min<unsigned long long>(n_pairs / kXLongRun + 1, 512);
      hipLaunchKernelGGL(k_apply_xlong_batch<MODE>, dim3(xb), dim3(256), 0, sx, F, n_pairs, (const uint64_t*)sp, tab, c->table, c->pool,
                         (const uint32_t*)c->d_label_lut.get(), (const unsigned long long*)d_xlong_list, (const uint32_t*)&C->n_xlong);
    }
    const uint32_t lb = (uint32_t)std::min<unsigned long long>(n_pairs / kLongRun + 1, 4096);
    hipLaunchKernelGGL(k_apply_long_batch<MODE>, dim3(lb), dim3(128), 0, sl, F, n_pairs, (const uint64_t*)sp, tab, c->table, c->pool,
                       (const uint32_t*)c->d_label_lut.get(), (const unsigned long long*)d_long_list, (const Counters*)C);
  }
};
#undef KS_LAUNCH_TIMED_IF
// The frame's n_pairs updates into the map: sorted by voxel, then k_apply with the long and xlong runs forked off beside it
int enqueue_update(ks_ctx* c, FrameSlot& S, hipStream_t st, unsigned long long n_pairs, uint32_t new_tiles, int set) {
  if (n_pairs == 0) {
    // a frame without updates still separates the frame before it from the one after it, which share a parity
    // buffer set: the long runs of the previous frame end before anything later is enqueued on the tail stream
    if (c->pending_join) HIPCHK(c, hipStreamWaitEvent(st, c->pending_join, 0));
    c->pending_join = nullptr;
    skip_update_stages(c, set);
    return KS_OK;
  }
  const FrameParams& F = S.F;
  int rc;
  if ((rc = ensure_pairs_out(c, n_pairs))) return rc;
  stage_mark(c, set, 7);
  const unsigned end_bit = F.seq_bits + 9 + bits_for(new_tiles);
  uint64_t* sp = nullptr;
  // k_emit wrote the pairs in integration order; the stable sort only groups them by voxel (it skips
  // the sequence bits), so every voxel replays its updates in the reference's single-thread order.
  const int par = (int)(S.frame_no & 1u);
  // (the update before this one used the same set — a batch's tail, or a frame that was not applied, lies between: its long runs
  // end before the sort writes into the set)
  if (par == c->last_par && c->pending_join) {
    HIPCHK(c, hipStreamWaitEvent(st, c->pending_join, 0));
    c->pending_join = nullptr;
  }
  c->last_par = par;
  unsigned long long* const d_long_list = c->d_long_list_[par];
  if ((rc = sort_keys(c, S.d_pairs.get(), c->d_pairs2_[par].get(), n_pairs, std::min(56u, end_bit), &sp, F.seq_bits, /*tail=*/true))) return rc;
  stage_mark(c, set, 8);
  const bool by_runs = n_pairs >= c->apply_runs_min_pairs;
  const bool time_apply = set >= 0 && c->pset[set].apply;
  if (time_apply) {
    c->pset[set].applied = true;
    c->pset[set].n_applied = n_pairs;
  }
  // long runs (voxels next to the sensor) are listed first; then the two update kernels run side by side:
  // k_apply on the tail stream, k_apply_long on its own stream (disjoint voxels)
  hipStream_t sl = c->stream_long, sx = c->stream_xlong;
  // Where the stream plan folds a side chain, its handle IS the tail stream: its kernels follow k_apply in stream order,
  // which is the order every fork and join below stands for, so those events are neither recorded nor waited for (and the
  // deferred join has nothing to defer: the next frame's sort simply follows on the same stream).
  const bool long_beside = sl != st, xlong_beside = sx && sx != st;
  unsigned long long* const d_xlong_list = sx ? d_long_list + (c->cap_pairs / kLongRunLanes + 64) : nullptr;
  const bool lanes_on = by_runs && sx && c->long_lanes && n_pairs >= c->long_lanes_min_pairs;
  // ("long" could begin at kLongRunLanes = 17 updates where the lanes kernel takes the long runs — k_find_long, k_long_measure and
  // k_apply_runs take the threshold as an argument — but measured at 1280x720 / 2 cm it buys nothing: k_apply_runs 2.83 vs 2.79 ms,
  // the lanes kernel 1.47 vs 0.93 ms, the frame 6.42 vs 6.24 ms: profiles/r06_c4_merged_ab.txt.)
  // k_apply_runs decides which runs are its own by itself: the listing of the long runs (a pass over all pairs, 0.3 ms at
  // 1280x720 / 2 cm) then runs BESIDE it, on the long-run stream, instead of in front of it
  // (only where both side chains have streams of their own: on the tail stream it would run in front of k_apply_runs anyway)
  const bool find_beside = by_runs && xlong_beside && long_beside;
  const dim3 find_grid((uint32_t)((n_pairs + 256 * kFindLongItems - 1) / (256 * kFindLongItems)));
  if (!find_beside)
    hipLaunchKernelGGL(k_find_long, find_grid, dim3(256), 0, st, F.seq_bits, n_pairs, (const uint64_t*)sp, d_long_list, d_xlong_list,
                       S.d_counters, kLongRun);
  // the previous frame's long runs end before any voxel of this frame is touched
  if (c->pending_join) HIPCHK(c, hipStreamWaitEvent(st, c->pending_join, 0));
  c->pending_join = nullptr;
  if (long_beside || xlong_beside) HIPCHK(c, hipEventRecord(S.fork, st));
  if (long_beside) HIPCHK(c, hipStreamWaitEvent(sl, S.fork, 0));
  if (lanes_on) HIPCHK(c, hipMemsetAsync(c->d_long_hdr_[par], 0, sizeof(LongHdr), sl));
  if (find_beside) {
    hipLaunchKernelGGL(k_find_long, find_grid, dim3(256), 0, sl, F.seq_bits, n_pairs, (const uint64_t*)sp, d_long_list, d_xlong_list,
                       S.d_counters, kLongRun);
    HIPCHK(c, hipEventRecord(S.found, sl));
    HIPCHK(c, hipStreamWaitEvent(sx, S.found, 0));
  } else if (xlong_beside) {
    HIPCHK(c, hipStreamWaitEvent(sx, S.fork, 0));
  }
  const UpdateLaunch U{c, S, F, st, sl, sx, set, par, sp, n_pairs, d_long_list, d_xlong_list, by_runs, time_apply, lanes_on};
  switch (c->cfg.color_mode) {
    case KS_COLOR_MODE_COLOR: U.launch<KS_COLOR_MODE_COLOR>(); break;
    case KS_COLOR_MODE_SEMANTIC: U.launch<KS_COLOR_MODE_SEMANTIC>(); break;
    default: U.launch<KS_COLOR_MODE_SEMANTIC_PROBABILITY>(); break;
  }
  if (xlong_beside) {  // S.join stands for both lists
    HIPCHK(c, hipEventRecord(S.join_x, sx));
    HIPCHK(c, hipStreamWaitEvent(sl, S.join_x, 0));
  }
  if (long_beside) {
    HIPCHK(c, hipEventRecord(S.join, sl));
    S.join_recorded = true;
    // deferred: the tail stream goes on with the next frame's tile initialisation, pair sort and long-run
    // listing (none of which touches voxels or this frame's buffer set) and waits before its k_apply
    if (!(set >= 0 && c->pset[set].stages)) c->pending_join = S.join;
    else HIPCHK(c, hipStreamWaitEvent(st, S.join, 0));
  }   // (else: the long runs are on the tail stream, and S.tail_done below stands for them too)
  return KS_OK;
}

// ---- the tail of a whole batch in one pass ----
// Whether a batch's tail may run as one pass: a pure function of what the frames' snapshots say (ks_tail_batch_rule).  Every
// frame must be one the per-frame tail would simply sort and apply through k_apply: no error bit (a label out of range, a
// fix point that fell back, pairs that did not fit: the frame is reported or repaired at its own call), fewer pairs than
// k_apply_runs and the integer-sum path of the xlong runs start at; not a marcher, not under the stage profile.
bool tail_batch_rule(const uint32_t* err, const unsigned long long* n_pairs, int nb, bool marcher, int profiling, unsigned long long runs_min_pairs,
                     unsigned long long xl_min_pairs) {
  if (nb < 2 || nb > kBatchMax || marcher || profiling == 1) return false;
  unsigned long long total = 0;
  for (int k = 0; k < nb; ++k) {
    if (err[k] || n_pairs[k] >= runs_min_pairs || n_pairs[k] >= xl_min_pairs) return false;
    total += n_pairs[k];
  }
  return total > 0;
}
int ensure_tail_batch(ks_ctx* c, size_t n) {
  int rc;
  for (int b = 0; b < 2; ++b)
    if (!c->d_tail_frames_[b] && (rc = c->d_tail_frames_[b].alloc(c, kBatchMax))) return rc;
  if (n <= c->cap_cat) return KS_OK;
  const size_t cap = std::max<size_t>(n + n / 4, 1 << 20);
  c->cap_cat = 0;
  HIPCHK(c, hipStreamSynchronize(c->stream_long));  // (as ensure_pairs_out: the sorted pairs of the batch before may be in one of them)
  if (c->stream_xlong) HIPCHK(c, hipStreamSynchronize(c->stream_xlong));
  if (c->stream_tail) HIPCHK(c, hipStreamSynchronize(c->stream_tail));
  for (int b = 0; b < 2; ++b)
    if ((rc = c->d_pairs_cat_[b].alloc(c, cap))) return rc;
  c->cap_cat = cap;
  return KS_OK;
}
// Called by the tail of a batch's FIRST frame (S0; its snapshot has landed).  Stage B of a batch is one launch sequence and its
// frames finish together, so the pairs of every frame of the batch are on the device by now.  Where the rule allows it, ONE
// sort and ONE voxel update take them all: the lists go one behind the other in frame order, the stable sort groups them by
// voxel and skips the sequence field — ray sequence and, above it, the frame's index — so that every voxel replays its
// updates in (frame, integration position) order: the record is bit for bit what one pass per frame leaves, and the map is
// read and written once instead of once per frame.  Each frame's slot is marked (tail_batched); its own frame_tail call then
// only accounts for it.  Otherwise nothing is done here and every frame's tail runs on its own, as it does without batches.
int tail_batch(ks_ctx* c, FrameSlot& S0) {
  const int nb = S0.batch_nb;
  FrameSlot* const* slots = S0.batch_slots;
  if (nb < 2 || !S0.F.frame_bits) return KS_OK;   // (nothing to share, or keys without frame bits)
  int rc;
  if (!c->tail_batch_on) {
    c->tb_stats[2] += 1;
    return KS_OK;
  }
  hipStream_t st = c->stream_tail;
  HIPCHK(c, hipEventSynchronize(slots[nb - 1]->ready));   // (recorded behind the batch's last launch, like every slot's)
  uint32_t err[kBatchMax];
  unsigned long long np[kBatchMax], total = 0;
  bool same_keys = true;
  for (int k = 0; k < nb; ++k) {
    err[k] = slots[k]->counters().err;
    np[k] = slots[k]->counters().n_pairs;
    total += np[k];
    same_keys = same_keys && (k == 0 || slots[k]->pending) && slots[k]->F.seq_bits == S0.F.seq_bits && (slots[k]->F.frame_bits & 0xffu) == (S0.F.frame_bits & 0xffu);
  }
  if (!same_keys || !tail_batch_rule(err, np, nb, c->shard_export, c->profiling, c->apply_runs_min_pairs,
                                     c->stream_xlong && c->xl_parallel ? c->xl_min_pairs : ~0ull)) {
    c->tb_stats[2] += 1;
    return KS_OK;
  }
  // the tiles the batch's fronts allocated: valid before anything is applied; each frame's share as its own tail would count it
  uint32_t tiles = c->tiles_initialised;
  for (int k = 0; k < nb; ++k) {
    const uint32_t nt = std::min(slots[k]->n_tiles(), c->cfg.max_tiles);
    slots[k]->tb_blocks = nt > tiles ? nt - tiles : 0u;
    tiles = std::max(tiles, nt);
  }
  if (tiles > c->tiles_initialised) {
    hipLaunchKernelGGL(k_init_tiles, dim3(tiles - c->tiles_initialised), dim3(512), 0, st, c->pool, c->tiles_initialised);
    c->tiles_initialised = tiles;
  }
  if ((rc = ensure_pairs_out(c, total)) || (rc = ensure_tail_batch(c, total))) return rc;
  const int par = c->last_par == 0 ? 1 : 0;   // the set the update before this one did not use
  c->last_par = par;
  const FrameParams& F = S0.F;   // (the configuration: the same for every frame of the batch)
  TailFrames TF{};
  PairLists L{};
  unsigned long long longest = 0;
  for (int k = 0; k < kBatchMax; ++k) {
    const FrameSlot& S = *slots[std::min(k, nb - 1)];   // (entries past the batch repeat its last frame: no key names them)
    TF.f[k].rays = S.d_rays;
    TF.f[k].t = S.F.T.t;
    TF.f[k].point_mask = S.F.point_mask;
    TF.f[k].order_groups = S.F.order_groups;
    TF.f[k].order_per = S.F.order_per;
    L.src[k] = S.d_pairs;
    L.off[k + 1] = L.off[k] + (k < nb ? np[k] : 0ull);
    longest = std::max(longest, k < nb ? np[k] : 0ull);
  }
  TailFrame* const tab = c->d_tail_frames_[par];
  hipLaunchKernelGGL(k_set_tail_frames, dim3(kBatchMax), dim3(64), 0, st, TF, tab);
  hipLaunchKernelGGL(k_cat_pairs, dim3((uint32_t)std::min<unsigned long long>((longest + 1023) / 1024, 2048), (uint32_t)nb), dim3(256), 0, st, L,
                     c->d_pairs_cat_[par].get());
  const unsigned end_bit = F.seq_bits + 9 + bits_for(tiles);
  uint64_t* sp = nullptr;
  if ((rc = sort_keys(c, c->d_pairs_cat_[par].get(), c->d_pairs2_[par].get(), total, std::min(56u, end_bit), &sp, F.seq_bits, /*tail=*/true))) return rc;
  // from here on as enqueue_update: the long runs listed, then the three kernels side by side where the plan gives them streams
  hipStream_t sl = c->stream_long, sx = c->stream_xlong;
  const bool long_beside = sl != st, xlong_beside = sx && sx != st;
  unsigned long long* const d_long_list = c->d_long_list_[par];
  unsigned long long* const d_xlong_list = sx ? d_long_list + (c->cap_pairs / kLongRunLanes + 64) : nullptr;
  const dim3 find_grid((uint32_t)((total + 256 * kFindLongItems - 1) / (256 * kFindLongItems)));
  hipLaunchKernelGGL(k_find_long, find_grid, dim3(256), 0, st, F.seq_bits, total, (const uint64_t*)sp, d_long_list, d_xlong_list, S0.d_counters, kLongRun);
  if (c->pending_join) HIPCHK(c, hipStreamWaitEvent(st, c->pending_join, 0));
  c->pending_join = nullptr;
  if (long_beside || xlong_beside) HIPCHK(c, hipEventRecord(S0.fork, st));
  if (long_beside) HIPCHK(c, hipStreamWaitEvent(sl, S0.fork, 0));
  if (xlong_beside) HIPCHK(c, hipStreamWaitEvent(sx, S0.fork, 0));
  int timed = -1;   // level-2 profile: the batch's k_apply carries the events of its first frame that is due for them
  for (int k = 0; k < nb && timed < 0; ++k)
    if (slots[k]->prof_set >= 0 && c->pset[slots[k]->prof_set].apply) timed = slots[k]->prof_set;
  if (timed >= 0) {
    c->pset[timed].applied = true;
    c->pset[timed].n_applied = total;
  }
  const BatchUpdateLaunch U{c, F, st, sl, sx, timed, sp, total, d_long_list, d_xlong_list, tab, S0.d_counters};
  switch (c->cfg.color_mode) {
    case KS_COLOR_MODE_COLOR: U.launch<KS_COLOR_MODE_COLOR>(); break;
    case KS_COLOR_MODE_SEMANTIC: U.launch<KS_COLOR_MODE_SEMANTIC>(); break;
    default: U.launch<KS_COLOR_MODE_SEMANTIC_PROBABILITY>(); break;
  }
  if (xlong_beside) {
    HIPCHK(c, hipEventRecord(S0.join_x, sx));
    HIPCHK(c, hipStreamWaitEvent(sl, S0.join_x, 0));
  }
  // every slot of the batch is free for stage A once the batch's update has read its rays (and its long runs have ended)
  for (int k = 0; k < nb; ++k) {
    FrameSlot& S = *slots[k];
    if (long_beside) {
      HIPCHK(c, hipEventRecord(S.join, sl));
      S.join_recorded = true;
    }
    HIPCHK(c, hipEventRecord(S.tail_done, st));
    S.tail_recorded = true;
    S.tail_batched = true;
  }
  if (long_beside) c->pending_join = S0.join;   // deferred, as in enqueue_update
  HIPCHK(c, hipGetLastError());
  c->tb_stats[0] += 1;
  c->tb_stats[1] += (uint64_t)nb;
  c->tb_stats[3] += total;
  return KS_OK;
}

int frame_tail(ks_ctx* c, FrameSlot& S) {
  if (!S.pending) return KS_OK;
  S.pending = false;
  // After a pool / index failure the table may hold entries without a tile: frames that were
  // already in flight are dropped, never applied (the error has been reported for the frame that hit it).
  if (c->fatal) return KS_OK;
  int rc;
  // (the frame's batch has not filled up — a flush, or a lag shorter than the batch: it goes out as it is)
  if (!S.b_launched && (rc = launch_batch(c))) return rc;
  hipStream_t st = c->stream_tail;  // the host wait below orders the tail after the slot's front
  const auto w0 = std::chrono::steady_clock::now();
  HIPCHK(c, hipEventSynchronize(S.ready));  // the frame's only host wait
  // the first frame of a batch decides for all of them whether the batch's tail is one pass
  if (S.batch_index == 0 && (rc = tail_batch(c, S))) return rc;
  if (c->profiling) c->prof.host_wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
  Counters cnt = S.counters();
  uint32_t new_tiles = std::min(S.n_tiles(), c->cfg.max_tiles);
  const uint32_t tiles_before = c->tiles_initialised;
  const int set = S.prof_set;
  stage_mark(c, set, 6);
  if (c->eo_device && !c->eo_device_off) {
    c->eo_frames += 1;
    c->eo_iterations += S.h_snap->pad[2];   // rounds of the event-driven fix point (k_publish)
    if (!(cnt.err & kErrExact)) c->eo_hopeless.store(0, std::memory_order_relaxed);
  }
  if ((cnt.err & kErrExact) && !(cnt.err & (kErrLabel | kErrIndex)) && (rc = repair_after_fallback(c, S, st, &cnt, &new_tiles))) return rc;
  c->pairs_hint.store(std::max<size_t>(c->pairs_hint.load(std::memory_order_relaxed), cnt.n_pairs), std::memory_order_relaxed);
  if (S.tail_batched) {
    // applied with its batch (no error bit, tiles valid, events recorded: tail_batch): what is left is the frame's account
    S.tail_batched = false;
    skip_update_stages(c, set);
    finish_prof(c, set, st, cnt.n_pairs);
    owe_stats(c, S, cnt, cnt.n_pairs, S.tb_blocks);
    return KS_OK;
  }
  if ((cnt.err & kErrPairs) && !(cnt.err & ~kErrPairs) && (rc = repair_after_overflow(c, S, st, &cnt, &new_tiles))) return rc;
  // tiles allocated by the front exist in the table whatever happens next: make them valid
  if (new_tiles > c->tiles_initialised) {
    hipLaunchKernelGGL(k_init_tiles, dim3(new_tiles - c->tiles_initialised), dim3(512), 0, st, c->pool, c->tiles_initialised);
    c->tiles_initialised = new_tiles;
  }
  if (cnt.err) return take_error_exits(c, set, st, cnt.err);
  const unsigned long long n_pairs = cnt.n_pairs;
  // a marcher of ks_integrate_round_exact: the frame's updates leave as records, grouped by the rank that owns their tile
  const bool marcher = c->shard_export;
  if (marcher) skip_update_stages(c, set);
  if ((rc = marcher ? shard_export_frame(c, S, n_pairs, st) : enqueue_update(c, S, st, n_pairs, new_tiles, set))) return rc;
  finish_prof(c, set, st, n_pairs);
  HIPCHK(c, hipEventRecord(S.tail_done, st));
  S.tail_recorded = true;
  if (!marcher) HIPCHK(c, hipGetLastError());
  owe_stats(c, S, cnt, n_pairs, !marcher && new_tiles > tiles_before ? new_tiles - tiles_before : 0u);  // (marches of later frames run ahead)
  if (c->use_bundle_rank && !c->bo_hint_fixed && !marcher) {
    // the bundle count the next frames' epochs are launched for: this frame's rays (= bundles of both maps) + 25 % + 2048, decaying slowly
    const uint32_t want = cnt.n_rays + cnt.n_rays / 4u + 2048u;
    const uint32_t cur = c->bo_hint.load(std::memory_order_relaxed);
    c->bo_hint.store(cur == ~0u ? want : std::max(want, cur - cur / 64u), std::memory_order_relaxed);
  }
  return KS_OK;
}

// hand the statistics of every frame completed since the last hand-over to the caller
void deliver_stats(ks_ctx* c, ks_frame_stats* stats) {
  if (stats) *stats = c->owed;
  c->owed = ks_frame_stats{};
}

// run the tail of a frame whose front is still waiting for it (pipelined mode)
int flush_pending(ks_ctx* c) {
  // up to two slots are pending between calls; oldest frame first
  for (int k = 0; k < c->n_slots; ++k) {
    FrameSlot& S = c->slot[(c->frame_no + k) % (uint64_t)c->n_slots];
    if (S.pending) {
      const int rc = frame_tail(c, S);
      if (rc) return rc;
    }
  }
  return KS_OK;
}

int ensure_exchange(ks_ctx* c, size_t n) {
  if (n <= c->d_xchg_u64.size()) return KS_OK;
  const size_t cap = std::max<size_t>(n + n / 2, 1024);
  c->d_xchg_u64.release();   // (its size stands for both)
  if (int rc = c->d_xchg_u32.alloc(c, 2 * cap + 2)) return rc;
  return c->d_xchg_u64.alloc(c, cap);
}

// complete every outstanding frame and drain both streams
int quiesce(ks_ctx* c) {
  const int rc = flush_pending(c);
  if (c->stream_tail != c->stream) HIPCHK(c, hipStreamSynchronize(c->stream_tail));
  HIPCHK(c, hipStreamSynchronize(c->stream_long));
  c->pending_join = nullptr;
  if (int rc2 = sync_march(c)) return rc2;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return rc;
}

void tail_worker(ks_ctx* c) {
  (void)hipSetDevice(c->cfg.device_id);
  std::unique_lock<std::mutex> lk(c->tail_mu);
  for (;;) {
    c->tail_cv.wait(lk, [&] { return c->tail_job != nullptr || c->tail_quit; });
    if (c->tail_quit) return;
    FrameSlot* S = c->tail_job;
    c->tail_job = nullptr;
    lk.unlock();
    int rc;
    {
      std::lock_guard<std::mutex> cap(c->capture_mu);
      rc = frame_tail(c, *S);
    }
    lk.lock();
    c->tail_rc = rc;
    c->tail_busy = false;
    c->tail_cv.notify_all();
  }
}
void tail_post(ks_ctx* c, FrameSlot* S) {
  std::lock_guard<std::mutex> lk(c->tail_mu);
  c->tail_job = S;
  c->tail_busy = true;
  c->tail_rc = KS_OK;
  c->tail_cv.notify_all();
}
int tail_join(ks_ctx* c) {
  std::unique_lock<std::mutex> lk(c->tail_mu);
  c->tail_cv.wait(lk, [&] { return !c->tail_busy; });
  return c->tail_rc;
}

// The reference allocates blocks on demand without a cap [K:src/semantic_integrator_base.cpp:205-254]; the tile
// pool here is one allocation.  When more than half of it is in use it is doubled between frames (new
// allocation, device-to-device copy of the tiles in use, table rebuilt with the same slot numbers), so a map
// only stops growing when HBM is exhausted.  ks_config.max_tiles is the INITIAL capacity.
int grow_pool(ks_ctx* c) {
  int rc;
  if ((rc = quiesce(c))) return rc;
  const size_t old_max = c->cfg.max_tiles;
  const size_t new_max = std::min<size_t>(old_max * 2, (1u << 23) - 1);
  if (new_max <= old_max) return KS_OK;
  const uint32_t nt = c->tiles_initialised;
  DevBuf<uint4> vox;
  DevBuf<uint8_t> upd, dirty;
  DevBuf<uint64_t> skeys;
  DevBuf<TileEntry> ent;
  uint32_t cap = 1024;
  while (cap < 2u * new_max) cap <<= 1;
  if (vox.try_alloc(new_max * kTileVoxels * 8) != hipSuccess) {
    (void)hipGetLastError();
    return KS_OK;  // no memory for a bigger pool: carry on with the current one (exhaustion is reported when it happens)
  }
  // (a failure part-way leaves the old pool in place; the locals free what was allocated for the new one)
  if ((rc = upd.alloc(c, kFlagPlane + new_max))) return rc;   // two planes: updated | mesh_stale
  if ((rc = dirty.alloc(c, new_max))) return rc;
  if ((rc = skeys.alloc(c, new_max))) return rc;
  if ((rc = ent.alloc(c, cap))) return rc;
  HIPCHK(c, hipMemset(upd, 0, new_max));
  HIPCHK(c, hipMemset(dirty, 0, new_max));
  HIPCHK(c, hipMemset(upd + kFlagPlane, 0, new_max));
  HIPCHK(c, hipMemset(ent, 0xff, (size_t)cap * sizeof(TileEntry)));
  if (nt) {
    HIPCHK(c, hipMemcpy(vox, c->pool.vox, (size_t)nt * kTileVoxels * 8 * sizeof(uint4), hipMemcpyDeviceToDevice));
    HIPCHK(c, hipMemcpy(upd, c->pool.updated, nt, hipMemcpyDeviceToDevice));
    HIPCHK(c, hipMemcpy(dirty, c->pool.dirty, nt, hipMemcpyDeviceToDevice));
    HIPCHK(c, hipMemcpy(upd + kFlagPlane, c->pool.mesh_stale(), nt, hipMemcpyDeviceToDevice));
    HIPCHK(c, hipMemcpy(skeys, c->table.slot_keys, (size_t)nt * sizeof(uint64_t), hipMemcpyDeviceToDevice));
  }
  c->pool.vox = c->pool_vox = std::move(vox);
  c->pool.updated = c->pool_updated = std::move(upd);
  c->pool.dirty = c->pool_dirty = std::move(dirty);
  c->table.slot_keys = c->table_slot_keys = std::move(skeys);
  c->table.ent = c->table_ent = std::move(ent);
  c->table.mask = cap - 1;
  c->table.max_tiles = (uint32_t)new_max;
  c->cfg.max_tiles = (uint32_t)new_max;
  if (nt) hipLaunchKernelGGL(k_rehash_tiles, dim3((nt + 255) / 256), dim3(256), 0, c->stream, c->table, (const uint64_t*)c->table.slot_keys, nt);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  ++c->buffers_epoch;  // captured graphs hold the old table / pool
  return KS_OK;
}

int integrate_device_impl(ks_ctx* c, const float Tq[7], const float* d_xyz, const uint8_t* d_rgba, const uint8_t* d_labels,
                          size_t n, int freespace, ks_frame_stats* stats) {
  if (c->fatal) {
    c->err = "context is in a failed state (earlier pool/index error)";
    return KS_ERR_INVALID_ARG;
  }
  if (n >= (1u << 23)) {
    c->err = "more than 2^23-1 points per call";
    return KS_ERR_INVALID_ARG;
  }
  if (c->uses_early_out && n > kObsMaxPoints) {
    c->err = "fast integrator with the early-out enabled: at most 2^22-2 points per call";
    return KS_ERR_UNSUPPORTED;
  }
  const ks_config& cfg = c->cfg;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  int rc;
  if (c->eo_device && !c->eo_device_off && c->eo_hopeless.load(std::memory_order_relaxed) >= 3) {
    // the device loop keeps giving up on this context's frames: the host-driven loop from here on, one frame at a time
    if ((rc = quiesce(c))) return rc;
    c->eo_device_off = true;
    c->cfg.pipeline_frames = 0;
  }
  // sorted integration order keeps its permutation in single buffers: not pipelined
  bool pipelined = cfg.pipeline_frames && cfg.integration_order_mode != KS_ORDER_SORTED;
  if (pipelined && c->eo_device && !c->eo_device_off) {
    // A frame that fell back enters its marks when its tail runs, `pipeline_frames` calls after its stage B — so the frames
    // in flight behind it find their predecessor's marks missing when their finisher runs and follow it to the host-driven
    // loop, and so would every frame after them, for ever.  Complete what is in flight once and start afresh.
    const uint64_t fb = c->eo_fallbacks.load(std::memory_order_relaxed);
    if (fb != c->eo_fallbacks_seen) {
      if ((rc = quiesce(c))) return rc;
      c->eo_fallbacks_seen = c->eo_fallbacks.load(std::memory_order_relaxed);
    }
  }

  // frame-level bookkeeping of the fast integrator [K:src/semantic_tsdf_integrator_fast.cpp:165-170]
  if (cfg.method == KS_METHOD_FAST) {
    if ((++c->reset_counter) >= cfg.clear_checks_every_n_frames) {
      c->reset_counter = 0;
      if ((rc = reset_set(c, c->d_start_set, &c->start_offset, false))) return rc;
      if ((rc = reset_set(c, nullptr, &c->observed_offset, true))) return rc;
    }
    ++c->obs_tag;  // this frame's marks
  }
  if (n == 0) {
    if ((rc = quiesce(c))) return rc;
    deliver_stats(c, stats);
    return KS_OK;
  }
  {
    // freshest tile count the host has seen (snapshots of frames whose tail is still to come included)
    uint32_t known = c->tiles_initialised;
    for (const FrameSlot& S2 : c->slot)
      if (S2.h_snap) known = std::max(known, S2.h_snap->n_tiles);
    if ((size_t)known * 2 > (size_t)c->cfg.max_tiles && (rc = grow_pool(c))) return rc;
  }
  if (n > c->cap_points) {  // growing frees buffers a pending tail still needs
    if ((rc = quiesce(c))) return rc;
    if ((rc = ensure_points(c, n))) return rc;
  }
  if (c->eo_device && !c->eo_device_off) {
    if (c->eo_want_marks.load(std::memory_order_relaxed) > c->eo_cap_marks || c->eo_want_x.load(std::memory_order_relaxed) > c->eo_cap_x) {
      if ((rc = quiesce(c))) return rc;   // (the frames in flight may ask for more while they are completed)
      const size_t wm = std::max(c->eo_want_marks.load(std::memory_order_relaxed), c->eo_cap_marks);
      // (a frame that wants more X marks than an eighth of its marks is not helped by room for them — frame_tail counts it
      // as hopeless — so the X buffers never need more than that)
      const size_t wx = std::max(std::min(c->eo_want_x.load(std::memory_order_relaxed), std::max<size_t>(wm / 8, (size_t)1 << 17)), c->eo_cap_x);
      if (ensure_exact_slots(c, wm, wx) != KS_OK) {
        // no memory for it: this context stays with the host-driven loop (one frame at a time, the buffers of ensure_marks)
        // instead of failing the frame.  The slots' buffers may be gone: nothing of the event-driven path is touched again.
        (void)hipGetLastError();
        c->eo_device_off = true;
        c->cfg.pipeline_frames = 0;
        c->batch = 1;          // (one frame at a time from here on — this frame included: nothing is in flight after the quiesce above)
        pipelined = false;
        c->err.clear();
      }
      c->eo_want_x.store(0, std::memory_order_relaxed);   // (what was asked for has been looked at: a clamped request must not come back every frame)
      c->eo_fallbacks_seen = c->eo_fallbacks.load(std::memory_order_relaxed);
    }
    if (const int wb = c->eo_want_bulk.load(std::memory_order_relaxed); wb > c->eo_bulk_rounds) {
      if ((rc = quiesce(c))) return rc;   // (the helper thread reads eo_bulk_rounds while it runs a tail)
      c->eo_bulk_rounds = wb;
      ++c->buffers_epoch;                 // the captured launch sequences hold the old number of rounds
    }
  }
  if (!pipelined) {
    if ((rc = quiesce(c))) return rc;
    FrameSlot& S = c->slot[0];
    if ((rc = frame_front(c, S, Tq, d_xyz, d_rgba, d_labels, n, freespace))) return rc;
    rc = frame_tail(c, S);
    deliver_stats(c, stats);
    return rc;
  }
  // pipelined: stages A and B of this frame first, then stage T of the frame `lag` calls back
  // (its snapshot is long there: the host never waits for the march that is still running, and the
  // next call can enqueue stage A while this frame's march is in flight); the statistics returned
  // are those of the frames completed here
  const uint64_t lag = (uint64_t)std::min(std::max(cfg.pipeline_frames, 1), kMaxLag);
  FrameSlot& S = c->slot[c->frame_no % (uint64_t)c->n_slots];
  if (S.pending && (rc = frame_tail(c, S))) return rc;  // cannot happen: the slot's frame is 4 calls old
  const uint64_t this_frame = c->frame_no;
  FrameSlot* due = (this_frame >= lag) ? &c->slot[(this_frame - lag) % (uint64_t)c->n_slots] : nullptr;
  if (due && !due->pending) due = nullptr;
  if (due && !due->b_launched && (rc = launch_batch(c))) return rc;  // (only with a lag shorter than the batch)
  if (due && c->use_tail_thread) {
    tail_post(c, due);  // the helper thread enqueues the tail of the frame `lag` calls back ...
    const int rc_front = frame_front(c, S, Tq, d_xyz, d_rgba, d_labels, n, freespace);  // ... while this one enqueues A and B
    rc = tail_join(c);
    if (rc_front) rc = rc_front;
  } else {
    if ((rc = frame_front(c, S, Tq, d_xyz, d_rgba, d_labels, n, freespace))) return rc;
    if (due) rc = frame_tail(c, *due);
  }
  deliver_stats(c, stats);
  return rc;
}

int integrate_device(ks_ctx* c, const float Tq[7], const float* d_xyz, const uint8_t* d_rgba, const uint8_t* d_labels,
                     size_t n, int freespace, ks_frame_stats* stats) {
  if (!c->profiling) return integrate_device_impl(c, Tq, d_xyz, d_rgba, d_labels, n, freespace, stats);
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = integrate_device_impl(c, Tq, d_xyz, d_rgba, d_labels, n, freespace, stats);
  c->prof.host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

// ---- what the readers of the finished map share (block lists, mesh, ESDF) ----
void sort_unique(std::vector<uint64_t>& v) {
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
}
// tile positions (pack_coord3 of tile coordinates) -> the words of their blocks (pack_coord3 of block indices), ascending (x, y, z) and unique
std::vector<uint64_t> blocks_of_tiles(const std::vector<uint64_t>& tile_pos, int vps_shift) {
  std::vector<uint64_t> blocks(tile_pos.size());
  for (size_t i = 0; i < tile_pos.size(); ++i) {
    int t[3];
    unpack_coord3(tile_pos[i], t[0], t[1], t[2]);
    blocks[i] = pack_coord3(t[0] >> vps_shift, t[1] >> vps_shift, t[2] >> vps_shift);
  }
  sort_unique(blocks);
  return blocks;
}
// packed words -> int32 triples, in the order given
void words_to_triples(const std::vector<uint64_t>& words, std::vector<int32_t>* out) {
  out->resize(3 * words.size());
  for (size_t i = 0; i < words.size(); ++i) unpack_coord3(words[i], (*out)[3 * i], (*out)[3 * i + 1], (*out)[3 * i + 2]);
}

// The tile directory of a quiesced context on the host: slot -> tile key, slot -> flag byte (a plane of Pool::updated).  A fetch is one blocking copy.
struct TileSnapshot {
  uint32_t nt;
  std::vector<uint64_t> keys;
  std::vector<uint8_t> flags;
  explicit TileSnapshot(const ks_ctx* c) : nt(c->tiles_initialised) {}
  int fetch_keys(ks_ctx* c) {   // (once: a second call finds them there)
    if (keys.size() == nt) return KS_OK;
    keys.resize(nt);
    HIPCHK(c, hipMemcpy(keys.data(), c->table.slot_keys, (size_t)nt * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return KS_OK;
  }
  int fetch_flags(ks_ctx* c, const uint8_t* d_plane) {
    flags.resize(nt);
    if (nt) HIPCHK(c, hipMemcpy(flags.data(), d_plane, nt, hipMemcpyDeviceToHost));
    return KS_OK;
  }
  void tile(uint32_t s, int t[3]) const { unpack_tile(keys[s], t[0], t[1], t[2]); }
  // the blocks (blocks_of_tiles) of the tiles from slot `first` on whose flag byte has a bit of `mask`; mask 0: of all of them.
  // The keys are fetched at the first such tile unless they are there: with no such tile they are not read at all
  int blocks(ks_ctx* c, int vps_shift, uint32_t first, uint8_t mask, std::vector<uint64_t>* out) {
    std::vector<uint64_t> tiles;
    for (uint32_t s = first; s < nt; ++s) {
      if (mask && !(flags[s] & mask)) continue;
      if (int rc = fetch_keys(c)) return rc;
      int t[3];
      tile(s, t);
      tiles.push_back(pack_coord3(t[0], t[1], t[2]));
    }
    *out = blocks_of_tiles(tiles, vps_shift);
    return KS_OK;
  }
};

// ks_num_blocks, ks_get_block_indices, ks_get_updated_block_indices: the blocks of all tiles, or of those flagged `updated`
int collect_block_indices(ks_ctx* c, bool only_updated, bool reset, int32_t* out, size_t cap, size_t* n) {
  if (!c || !n) return KS_ERR_INVALID_ARG;
  if (int rc = quiesce(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  TileSnapshot snap(c);
  if (int rc = snap.fetch_keys(c)) return rc;
  if (int rc = snap.fetch_flags(c, c->pool.updated)) return rc;
  if (snap.nt && only_updated && reset) HIPCHK(c, hipMemset(c->pool.updated, 0, snap.nt));
  std::vector<uint64_t> blocks;
  if (int rc = snap.blocks(c, c->vps_shift, 0, only_updated ? 0xff : 0, &blocks)) return rc;
  std::vector<int32_t> v;
  words_to_triples(blocks, &v);
  *n = v.size() / 3;
  if (out) std::memcpy(out, v.data(), std::min(cap, *n) * 3 * sizeof(int32_t));
  return KS_OK;
}

}  // namespace

// find-or-insert n tile keys (device array) and initialise the newly allocated tiles
static int insert_tiles(ks_ctx* c, const uint64_t* d_keys, size_t n, size_t distinct_at_most = ~(size_t)0) {
  int rc;
  if ((rc = quiesce(c))) return rc;
  // as for frames: keep at least half of the pool free for what is coming (all n keys may be new tiles — unless the caller knows
  // how many DISTINCT keys there can be: the records of a frame name a few thousand tiles a hundred times each)
  const size_t may_be_new = std::min(n, distinct_at_most);
  while ((size_t)c->tiles_initialised + may_be_new > (size_t)c->cfg.max_tiles / 2) {
    const uint32_t before = c->cfg.max_tiles;
    if ((rc = grow_pool(c))) return rc;
    if (c->cfg.max_tiles == before) break;  // at the limit, or no memory: exhaustion is reported if it happens
  }
  FrameSlot& S = c->slot[0];
  HIPCHK(c, hipMemsetAsync(S.d_counters, 0, sizeof(Counters), c->stream));
  hipLaunchKernelGGL(k_insert_tiles, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, c->table, S.d_counters,
                     d_keys, (uint32_t)n);
  {
    BatchView V{};
    V.s[0] = slot_view(S);
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, c->stream, V, (const uint32_t*)c->table.n_tiles);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint32_t new_tiles = std::min(S.n_tiles(), c->cfg.max_tiles);
  if (new_tiles > c->tiles_initialised) {
    hipLaunchKernelGGL(k_init_tiles, dim3(new_tiles - c->tiles_initialised), dim3(512), 0, c->stream, c->pool,
                       c->tiles_initialised);
    c->tiles_initialised = new_tiles;
  }
  if (S.counters().err) {
    c->fatal = true;
    c->err = "voxel tile pool exhausted: raise ks_config.max_tiles";
    return KS_ERR_POOL_FULL;
  }
  return KS_OK;
}

extern "C" {

int ks_default_config(ks_config* c) {
  if (!c) return KS_ERR_INVALID_ARG;
  std::memset(c, 0, sizeof(*c));
  c->voxel_size = 0.05f;
  c->voxels_per_side = 16;
  c->truncation_distance = 4 * 0.05f;
  c->max_weight = 10000.0f;
  c->min_ray_length_m = 0.1f;
  c->max_ray_length_m = 5.0f;
  c->voxel_carving_enabled = 1;
  c->use_const_weight = 0;
  c->allow_clear = 1;
  c->use_weight_dropoff = 1;
  c->use_sparsity_compensation_factor = 0;
  c->sparsity_compensation_factor = 1.0f;
  c->enable_anti_grazing = 0;
  c->start_voxel_subsampling_factor = 2.0f;
  c->max_consecutive_ray_collisions = 2;
  c->clear_checks_every_n_frames = 1;
  c->integration_order_mode = KS_ORDER_MIXED;
  c->integrator_threads = 1;
  c->method = KS_METHOD_FAST;
  c->bundle_order = KS_BUNDLE_ORDER_REFERENCE;
  c->semantic_measurement_probability = 0.9f;
  c->color_mode = KS_COLOR_MODE_SEMANTIC;
  c->n_dynamic_labels = 0;
  c->device_id = 0;
  c->max_tiles = 1u << 16;
  c->max_points = 1u << 20;
  return KS_OK;
}

int ks_create(const ks_config* cfg, ks_ctx** out) {
  if (!cfg || !out) {
    g_create_error = "null argument";
    return KS_ERR_INVALID_ARG;
  }
  const int vps = cfg->voxels_per_side;
  if (!(vps == 8 || vps == 16 || vps == 32 || vps == 64)) {
    g_create_error = "voxels_per_side must be 8, 16, 32 or 64";
    return KS_ERR_INVALID_ARG;
  }
  if (cfg->n_dynamic_labels < 0 || cfg->n_dynamic_labels > 32 || cfg->max_tiles == 0 || cfg->max_tiles >= (1u << 23)) {
    g_create_error = "bad n_dynamic_labels / max_tiles";
    return KS_ERR_INVALID_ARG;
  }
  // setSemanticProbabilities CHECKs [K:src/semantic_integrator_base.cpp:93-107]
  const float match = cfg->semantic_measurement_probability;
  const float non_match = 1.0f - cfg->semantic_measurement_probability;
  if (!(match > 0.0f) || !(non_match > 0.0f) || !(match < 1.0f) || !(non_match < 1.0f)) {
    g_create_error = "semantic_measurement_probability must be in (0,1)";
    return KS_ERR_PROBABILITY;
  }
  const float lm = std::log(match), lnm = std::log(non_match);  // host libm, as the reference
  if (!(lm > lnm)) {
    g_create_error = "log(p) must exceed log(1-p)";
    return KS_ERR_PROBABILITY;
  }
  if (cfg->early_out_phase_growth != 0 && cfg->early_out_phase_growth != KS_EARLY_OUT_EXACT &&
      (cfg->early_out_phase_growth < 16 || cfg->early_out_phase_growth > 4096)) {
    g_create_error = "early_out_phase_growth must be 0 / KS_EARLY_OUT_EXACT (the reference's serial result) or 16..4096 (ordered phases, growth in 1/16ths)";
    return KS_ERR_INVALID_ARG;
  }
  // the early-out can never fire if the threshold exceeds the longest possible ray
  const double max_steps = 3.0 * ((double)cfg->max_ray_length_m + 2.0 * cfg->truncation_distance) / (double)cfg->voxel_size + 8.0;
  const bool uses_early_out = (cfg->method == KS_METHOD_FAST) && ((double)cfg->max_consecutive_ray_collisions < max_steps);
  if (uses_early_out && (cfg->clear_checks_every_n_frames > 256)) {
    g_create_error = "fast integrator with the early-out enabled supports clear_checks_every_n_frames <= 256";
    return KS_ERR_UNSUPPORTED;
  }
  if (cfg->integration_order_mode != KS_ORDER_MIXED && cfg->integration_order_mode != KS_ORDER_SORTED &&
      cfg->integration_order_mode != KS_ORDER_MIXED_1024_GROUPS) {
    g_create_error = "integration_order_mode must be KS_ORDER_MIXED, KS_ORDER_SORTED or KS_ORDER_MIXED_1024_GROUPS";
    return KS_ERR_INVALID_ARG;
  }
  // (The runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues, default 4, and kernels of streams that share a queue
  // run one after the other; a pipelined context keeps up to seven streams busy and runs best with 8.  That is the HOST
  // PROCESS's setting, read by the HIP runtime when it initialises: the library does not touch the environment —
  // INTEGRATION.md 4.2 says where the embedding process sets it; bench.py and the demos do so before their first HIP call.)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device_id >= ndev) {
    g_create_error = "no HIP device (the MI355X path has no CPU fallback)";
    return KS_ERR_NO_DEVICE;
  }
  ks_ctx* c = new ks_ctx();
  c->cfg = *cfg;
  const bool want_exact = cfg->early_out_phase_growth == 0 || cfg->early_out_phase_growth == KS_EARLY_OUT_EXACT;
  c->exact_early_out = uses_early_out && want_exact;
  if (want_exact) {
    // the seed's schedule.  Any seed gives the same map (the fixed point is unique); what a finer one buys is fewer marks to
    // emit, sort and evaluate, what it costs is k_test launches.  Measured at 640x480 / 5 cm on rings of 40 / 20 frames
    // (profiles/r05_c2_seed_growth_ab.txt), ms per frame: 32 (12 phases) 0.575 / 0.487, 28: 0.559, 26: 0.533 / 0.467,
    // 24: 0.541 / 0.461, 22 (23 phases): 0.523 / 0.465, 20: 0.525 / 0.484, 18: 0.558 / 0.544; coarser ones lose more (64: +12 %),
    // and so does a longest phase of 64 / 96 / 128 generations on top of any of them (equal steps at the end: +1 ... +8 %).
    c->cfg.early_out_phase_growth = 22;
  }
  {
    const char* hl = dbg_env("KS_EXACT_HOST_LOOP");   // diagnostics / A-B: the host-driven fix-point loop of round 3 for every frame
    c->eo_device = c->exact_early_out && !(hl && hl[0] == '1');
    // The host-driven loop waits for the device per iteration: one frame at a time.  The event-driven fix point is
    // pipelined as long as a frame's marks are never seen by the next one (every frame bumps the set offset): what is left
    // of the dependence between frames — the zero-initialised slot — is carried by the commit events.
    if (c->exact_early_out && (!c->eo_device || c->cfg.clear_checks_every_n_frames > 1)) c->cfg.pipeline_frames = 0;
    const bool wide_rays = steps_max_of(c->cfg, (float)(1.0 / cfg->voxel_size)) > 400;
    // (long rays: a frame's marks cover whole rays — 2e8 marks of 33 bytes at 1280x720 / 2 cm — and a frame is tens of
    // milliseconds of GPU work: one frame at a time, one set of mark buffers)
    if (c->exact_early_out && wide_rays) c->cfg.pipeline_frames = 0;
    // (rounds the fix point needs from the doubling seed at 640x480 / 5 cm: 7 - 20 per frame over the bench trajectory, 9 - 12
    // on average.  A round that finds its list empty costs a launch of ~2 us; a round the ONE-workgroup finisher has to run in its
    // place costs ~0.1 ms: measured on a ring of 40 frames, 8 rounds as launches 0.681 ms/frame, 14 rounds 0.569
    // (profiles/r05_bulk_rounds_ab.txt).  A finisher that is handed too long a list asks for more: eo_want_bulk.)
    c->eo_bulk_rounds = wide_rays ? 32 : 20;
  }
  c->uses_early_out = uses_early_out;
  c->use_bundle_rank = cfg->method == KS_METHOD_MERGED && cfg->bundle_order == KS_BUNDLE_ORDER_REFERENCE;
  if (const char* bh = dbg_env("KS_BO_HINT")) {   // tests / A-B: a fixed bundle-count hint (0: as many as the frame has points)
    c->bo_hint_fixed = true;
    c->bo_hint.store(atoi(bh) > 0 ? (uint32_t)atoi(bh) : ~0u, std::memory_order_relaxed);
  }
  if (cfg->method == KS_METHOD_MERGED && !cfg->enable_anti_grazing) {
    // stage A groups the points by end voxel: a 32-bit key (the voxel relative to a window around the sensor that holds every
    // point within max_ray; anything else through a small hash table) sorts in four passes instead of the 64-bit key's eight.
    // Not with anti-grazing (its binary search wants the 64-bit keys in order), not for windows wider than 10 bits per axis.
    const double extent = 2.0 * std::ceil(((double)cfg->max_ray_length_m + 2.0 * (double)cfg->voxel_size) / (double)cfg->voxel_size) + 8.0;
    unsigned w = 1;
    while (w < 32 && (double)(1u << w) < extent) ++w;
    if (const char* kb = dbg_env("KS_KEY_WINDOW_BITS")) w = (unsigned)std::max(0, atoi(kb));   // tests: 1..10 = a window that small (the overflow path), 0 = 64-bit keys
    c->key_bits = (w >= 1 && w <= 10) ? w : 0;
  }
  c->log_match = lm;
  c->log_non_match = lnm;
  c->voxel_size_inv = (float)(1.0 / cfg->voxel_size);  // TsdfIntegratorBase::setLayer
  c->vps_shift = vps == 8 ? 0 : vps == 16 ? 1 : vps == 32 ? 2 : 3;
#define CRCHK(expr)                                                        \
  do {                                                                     \
    hipError_t e_ = (expr);                                                \
    if (e_ != hipSuccess) {                                                \
      g_create_error = std::string(#expr) + ": " + hipGetErrorString(e_);  \
      ks_destroy(c);                                                       \
      return KS_ERR_HIP;                                                   \
    }                                                                      \
  } while (0)
  // ... for a call that returns a KS_* code with its text in c->err (an owner's alloc / create)
#define CRKS(expr)                \
  do {                            \
    if ((expr) != KS_OK) {        \
      g_create_error = c->err;    \
      ks_destroy(c);              \
      return KS_ERR_HIP;          \
    }                             \
  } while (0)
  // the next stream of the context (creation order matters: below)
  auto new_stream = [c](hipStream_t* out) {
    Stream& s = c->streams[c->n_streams];
    if (int rc = s.create(c, hipStreamNonBlocking)) return rc;
    ++c->n_streams;
    *out = s;
    return (int)KS_OK;
  };
  CRCHK(hipSetDevice(cfg->device_id));
  CRKS(new_stream(&c->stream));
  // Frames in flight share nothing in stage B when a frame's early-out marks can never be seen by the next frame
  // (every frame bumps the set offset).  Then either (pipeline_frames < 8) every frame's stage B is its own launch
  // sequence and up to four of them run side by side on four streams, or (pipeline_frames = 8) stage B of four
  // consecutive frames is launched as ONE batch on one stream; each frame in flight has an early-out table of its
  // own.  Otherwise stage B stays strictly in frame order.
  const bool frames_independent = !uses_early_out || c->cfg.clear_checks_every_n_frames <= 1;
  c->batch = 1;
  if (const char* ov = dbg_env("KS_TEST_OVERLAP")) c->test_overlap = atoi(ov) != 0;   // diagnostics: the same schedule and result, rounds one after the other
  if (c->cfg.pipeline_frames >= 2 && frames_independent && (!c->exact_early_out || c->eo_device) && c->cfg.integration_order_mode != KS_ORDER_SORTED) {
    // (measured, 640x480: a batch of 4 behind 8 frames of lag ~ four single-frame sequences on four streams behind 4
    // frames of lag; batches of 2 or 3 lose to both: DESIGN.md)
    c->batch = c->cfg.pipeline_frames >= 16 ? 8 : c->cfg.pipeline_frames >= 8 ? 4 : 1;
  }
  // slots: the lag plus one batch being filled, a multiple of the batch (a batch then always starts on the same slots: its
  // captured launch sequence is found again)
  c->n_slots = !c->cfg.pipeline_frames ? 1 : (c->cfg.pipeline_frames > 8 || c->batch > 4) ? kSlots : 12;
  {
    // the runs of more than kXLongRun updates (the voxels next to the sensor) through a kernel of their own, four waves per run
    // (k_apply_xlong).  Same arithmetic, same order: the map does not change.  KS_XLONG=0 (diagnostics): one list, k_apply_long.
    const char* xp = dbg_env("KS_XLONG");
    c->xlong = xp ? atoi(xp) != 0 : true;
    StreamPlanIn in;
    in.uses_early_out = uses_early_out;
    in.exact_early_out = c->exact_early_out;
    in.frames_independent = frames_independent;
    in.pipeline_frames = c->cfg.pipeline_frames;
    in.batch = c->batch;
    in.xlong = c->xlong;
    in.budget = hw_queue_budget();
    c->plan = stream_plan(in);
  }
  {
    // The streams of the plan.  Creation order matters: the runtime spreads streams over its hardware queues in creation order,
    // and kernels of streams that share a hardware queue run one after the other, so the heavy chains (stage A, stage B,
    // stage T) come first and the light side chains of stage T LAST — where the plan leaves them streams of their own.
    // Without an early-out stage B is short (scan + emission): it follows stage A on the same stream.
    const StreamPlan& P = c->plan;
    c->n_march = P.n_march;
    for (int i = 0; i < P.n_march; ++i) {
      if (P.march_own) CRKS(new_stream(&c->stream_march_[i]));
      else c->stream_march_[i] = c->stream;
    }
    if (P.tail_own) CRKS(new_stream(&c->stream_tail));
    else c->stream_tail = c->stream;
    // a folded chain runs on the tail stream, in order behind k_apply: the same handle, created and destroyed once
    if (P.long_own) CRKS(new_stream(&c->stream_long));
    else c->stream_long = c->stream_tail;
    if (P.xlong_own) CRKS(new_stream(&c->stream_xlong));
    else if (c->xlong) c->stream_xlong = c->stream_tail;
    if (const char* ar = dbg_env("KS_APPLY_RUNS")) c->apply_runs_min_pairs = atoi(ar) ? 0ull : ~0ull;   // tests / A-B: always / never
    if (const char* tb = dbg_env("KS_TAIL_BATCH")) c->tail_batch_on = atoi(tb) != 0;   // tests / A-B: 0 = every frame's tail on its own (the same map)
    if (const char* ll = dbg_env("KS_LONG_LANES")) {   // A/B: 0 = k_apply_long (two wavefronts per run) for all of them, 2 = lanes for frames of any size (tests)
      c->long_lanes = atoi(ll) != 0;
      if (atoi(ll) == 2) c->long_lanes_min_pairs = 0ull;
    }
    if (c->long_lanes)
      for (int b = 0; b < 2; ++b) CRKS(c->d_long_hdr_[b].alloc(c, 1));
    if (const char* xl = dbg_env("KS_XL_PARALLEL")) {   // A/B: 0 = every such run through k_apply_xlong, 2 = the integer-sum path for frames of any size (tests)
      c->xl_parallel = atoi(xl) != 0;
      if (atoi(xl) == 2) c->xl_min_pairs = 0ull;
    }   // A/B: 0 = every such run through k_apply_xlong
    // tests: room for this many chunk summaries per frame (k_xl_number hands the runs that do not fit to k_apply_xlong)
    if (const char* xc = dbg_env("KS_XL_CAP_CHUNKS")) c->cap_xl_chunks = (uint32_t)std::max(1, atoi(xc));
    if (c->stream_xlong && c->xl_parallel) {
      CRKS(c->d_xl_runs.alloc(c, kXlMaxRuns));
      CRKS(c->d_xl_idx.alloc(c, kXlMaxRuns));
      CRKS(c->d_xl_hdr.alloc(c, 1));
      CRCHK(hipMemset(c->d_xl_hdr, 0, sizeof(XlHeader)));
      CRKS(c->d_xl_chunks.alloc(c, c->cap_xl_chunks));
    }
  }
  for (auto& P : c->pset) {
    for (auto& e : P.ev) CRKS(e.create(c, 0));   // (timing events)
    CRKS(P.k0.create(c, 0));
    CRKS(P.k1.create(c, 0));
  }
  uint32_t cap = 1024;
  while (cap < 2u * cfg->max_tiles) cap <<= 1;
  c->table.mask = cap - 1;
  c->table.max_tiles = cfg->max_tiles;
  const size_t mt = cfg->max_tiles;
  CRKS(c->table_ent.alloc(c, cap));
  CRKS(c->table_slot_keys.alloc(c, mt));
  c->table.ent = c->table_ent;
  c->table.slot_keys = c->table_slot_keys;
  CRCHK(hipMemset(c->table.ent, 0xff, cap * sizeof(TileEntry)));  // key = empty, val = kSlotPending
  CRKS(c->pool_vox.alloc(c, mt * kTileVoxels * 8));
  CRKS(c->pool_updated.alloc(c, kFlagPlane + mt));   // two planes: updated | mesh_stale (ks_types.h: Pool)
  CRKS(c->pool_dirty.alloc(c, mt));
  c->pool.vox = c->pool_vox;
  c->pool.updated = c->pool_updated;
  c->pool.dirty = c->pool_dirty;
  CRCHK(hipMemset(c->pool.updated, 0, mt));
  CRCHK(hipMemset(c->pool.dirty, 0, mt));
  CRCHK(hipMemset(c->pool.mesh_stale(), 0, mt));
  CRKS(c->d_start_set.alloc(c, (size_t)1 << kSetBits));
  c->n_obs = (uses_early_out && frames_independent) ? std::min(kObsTables, std::max(c->n_march, c->batch * c->n_march)) : 1;
  for (int t = 0; t < c->n_obs; ++t) {
    CRKS(c->d_observed_[t].alloc(c, (size_t)2 << kSetBits));   // {newest, older} per slot
    CRCHK(hipMemset(c->d_observed_[t], 0, 2 * (sizeof(uint64_t) << kSetBits)));
    CRCHK(hipMemcpy(c->d_observed_[t], &kObsPoison, 8, hipMemcpyHostToDevice));
  }
  CRCHK(hipMemset(c->d_start_set, 0, sizeof(uint64_t) << kSetBits));
  const uint64_t poison = ~0ull;  // ApproxHashSet ctor: slot[offset_=0] = SIZE_MAX
  CRCHK(hipMemcpy(c->d_start_set, &poison, 8, hipMemcpyHostToDevice));
  CRKS(c->d_retry_counters.alloc(c, 1));
  if (c->exact_early_out) {
    CRKS(c->d_eo_committed.alloc(c, 16));
    CRCHK(hipMemset(c->d_eo_committed, 0, 64));
    CRKS(c->d_eo_range.alloc(c, (size_t)1 << kSetBits));
    CRKS(c->d_eo_plain.alloc(c, (size_t)1 << kSetBits));
    CRCHK(hipMemset(c->d_eo_plain, 0, sizeof(uint64_t) << kSetBits));
    CRCHK(hipMemcpy(c->d_eo_plain, &poison, 8, hipMemcpyHostToDevice));  // ApproxHashSet ctor: slot[0] = SIZE_MAX
    CRKS(c->d_eo_state.alloc(c, 1));
    CRKS(c->h_eo_state.alloc(c, 1));
  }
  CRKS(c->d_label_lut.alloc(c, 256));
  CRCHK(hipMemcpy(c->d_label_lut, cfg->label_rgba, 1024, hipMemcpyHostToDevice));
  static_assert(sizeof(Counters) == 32, "snapshot layout");
  CRKS(c->d_state.alloc(c, 64 * (kSlots + 1)));
  CRCHK(hipMemset(c->d_state, 0, 64 * (kSlots + 1)));
  c->table.n_tiles = (uint32_t*)(c->d_state + 64 * kSlots);
  for (int i = 0; i < kSlots; ++i) {
    FrameSlot& S = c->slot[i];
    S.index = i;
    S.d_counters = (Counters*)(c->d_state + 64 * i);
    CRKS(S.h_snap.alloc(c, 1));
    CRKS(S.d_F.alloc(c, 1));
    std::memset(S.h_snap, 0, sizeof(HostSnap));
    for (Event* e : {&S.a_done, &S.ready, &S.tail_done, &S.fork, &S.join, &S.join_x, &S.found}) CRKS(e->create(c, hipEventDisableTiming));
  }
#undef CRKS
#undef CRCHK
  // pair buffers start at 4 updates per point of the largest cloud (a frame that needs more grows its buffer and
  // repeats the emission once)
  c->pairs_hint.store((size_t)cfg->max_points * 4, std::memory_order_relaxed);
  size_t eo_marks0 = std::max<size_t>((size_t)1 << 20, 4 * (size_t)cfg->max_points), eo_x0 = std::max<size_t>((size_t)1 << 17, (size_t)cfg->max_points);
  // long rays: the marks cover whole rays (measured at 1280x720 / 2 cm / 10 m: 250 marks per point of the cloud; room for a third of
  // the longest possible ray = ~10 GB there).  Asked for here, allocated by the first integrate call (the growth path at the top of
  // integrate_device_impl, before the frame is enqueued): a context that is created and never integrates (a map that is only loaded, merged into
  // or read back) does not hold it, and a device without the room falls back to the host-driven loop instead of failing
  // ks_create.
  size_t eo_marks_first = 0;
  if (c->exact_early_out && c->eo_device && steps_max_of(c->cfg, c->voxel_size_inv) > 400)
    eo_marks_first = (size_t)cfg->max_points * (steps_max_of(c->cfg, c->voxel_size_inv) / 3 + 32);
  // (tests: start small, so that the overflow -> host-driven loop -> grow path is exercised)
  if (const char* e = dbg_env("KS_EXACT_CAP_MARKS")) eo_marks0 = std::max<size_t>(64, (size_t)atoll(e)), eo_marks_first = 0;
  if (const char* e = dbg_env("KS_EXACT_CAP_X")) eo_x0 = std::max<size_t>(8, (size_t)atoll(e));
  // (tests: a seed launch that covers fewer items than a frame has — the frame must end in the error path, not lose rays)
  if (const char* e = dbg_env("KS_SEED_CAP_ITEMS")) c->seed_cap_items = std::max<size_t>(1, (size_t)atoll(e));
  // (tests: a host-pointer ESDF read of about a thousand points that crosses several chunk boundaries)
  if (const char* e = dbg_env("KS_ESDF_READ_CHUNK")) c->esdf_read_chunk = std::max<size_t>(1, (size_t)atoll(e));
  // (tests: host-pointer reads of the navigation field that cross several chunk boundaries)
  if (const char* e = dbg_env("KS_NAV_CHUNK")) c->nav_chunk = std::max<size_t>(1, (size_t)atoll(e));
  // (tests: views of a few thousand voxels on the global path, a box just below and above the budget; one bitmap reused by every view)
  if (const char* e = dbg_env("KS_VG_LDS_BITS")) c->vg_lds_bits = (uint32_t)std::min<long long>(std::max<long long>(0, atoll(e)), (long long)kVgLdsBits);
  if (const char* e = dbg_env("KS_VG_GROUPS")) c->vg_groups = (uint32_t)std::min<long long>(std::max<long long>(1, atoll(e)), (long long)kVgMaxGroups);
  // (tests: a host-pointer call that crosses several chunk boundaries; more paths than the grid has wavefronts)
  if (const char* e = dbg_env("KS_SHORTEN_CHUNK")) c->ps_chunk = std::max<size_t>(1, (size_t)atoll(e));
  if (const char* e = dbg_env("KS_SHORTEN_GRID")) c->ps_blocks = (uint32_t)std::min<long long>(std::max<long long>(1, atoll(e)), 4096);
  if (eo_marks_first > eo_marks0) c->eo_want_marks.store(eo_marks_first, std::memory_order_relaxed);
  if (ensure_points(c, cfg->max_points) != KS_OK || ensure_exact_slots(c, eo_marks0, eo_x0) != KS_OK) {
    g_create_error = c->err;
    ks_destroy(c);
    return KS_ERR_HIP;
  }
  c->use_tail_thread = c->cfg.pipeline_frames > 0;
  if (c->use_tail_thread) c->tail_thread = std::thread(tail_worker, c);
  *out = c;
  return KS_OK;
}

void ks_destroy(ks_ctx* c) {
  if (!c) return;
  if (c->tail_thread.joinable()) {
    {
      std::lock_guard<std::mutex> lk(c->tail_mu);
      c->tail_quit = true;
    }
    c->tail_cv.notify_all();
    c->tail_thread.join();
  }
  for (int i = 0; i < c->n_streams; ++i) (void)hipStreamSynchronize(c->streams[i]);   // every stream, before what its work refers to goes
  delete c;
}

const char* ks_last_error(ks_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int ks_set_color_to_label(ks_ctx* c, const uint8_t* rgba_keys, const uint8_t* labels, size_t n) {
  if (!c || (n && (!rgba_keys || !labels))) return KS_ERR_INVALID_ARG;
  // 16 MiB direct-mapped rgb -> label table; lookups force alpha = 255
  // ([K:src/semantic_tsdf_integrator_fast.cpp:157]), so only keys with alpha 255 can match
  // (HashableColor::operator== compares alpha, [K:src/color.cpp:25-27]); unknown -> 0.
  std::vector<uint8_t> lut(1u << 24, 0);
  for (size_t i = 0; i < n; ++i) {
    if (rgba_keys[4 * i + 3] != 255) continue;
    const uint32_t rgb = rgba_keys[4 * i] | (rgba_keys[4 * i + 1] << 8) | (rgba_keys[4 * i + 2] << 16);
    lut[rgb] = labels[i];
  }
  if (int rc = quiesce(c)) return rc;  // frames in flight still read the old table
  if (int rc = c->d_color_lut.reserve(c, 1u << 24, 1u << 24)) return rc;
  HIPCHK(c, hipMemcpy(c->d_color_lut, lut.data(), 1u << 24, hipMemcpyHostToDevice));
  return KS_OK;
}

int ks_integrate_points_device(ks_ctx* c, const float T[7], const float* d_xyz, const uint8_t* d_rgba,
                               const uint8_t* d_labels, size_t n, int freespace, ks_frame_stats* stats) {
  if (!c || !T || (n && !d_xyz)) return KS_ERR_INVALID_ARG;
  if (!d_labels && !(d_rgba && c->d_color_lut)) {
    c->err = "labels == NULL requires rgba and a colour map (ks_set_color_to_label)";
    return KS_ERR_INVALID_ARG;
  }
  return integrate_device(c, T, d_xyz, d_rgba, d_labels, n, freespace, stats);
}

int ks_integrate_points(ks_ctx* c, const float T[7], const float* xyz, const uint8_t* rgba, const uint8_t* labels,
                        size_t n, int freespace, ks_frame_stats* stats) {
  if (!c || !T || (n && !xyz)) return KS_ERR_INVALID_ARG;
  if (!labels && !(rgba && c->d_color_lut)) {
    c->err = "labels == NULL requires rgba and a colour map (ks_set_color_to_label)";
    return KS_ERR_INVALID_ARG;
  }
  int rc;
  if (n > c->cap_points && (rc = quiesce(c))) return rc;  // growing frees buffers a pending tail still needs
  if ((rc = ensure_points(c, n))) return rc;
  if (n) {
    HIPCHK(c, hipMemcpyAsync(c->d_xyz, xyz, n * 12, hipMemcpyHostToDevice, c->stream));
    if (rgba) HIPCHK(c, hipMemcpyAsync(c->d_rgba, rgba, n * 4, hipMemcpyHostToDevice, c->stream));
    if (labels) HIPCHK(c, hipMemcpyAsync(c->d_labels, labels, n, hipMemcpyHostToDevice, c->stream));
  }
  return integrate_device(c, T, c->d_xyz, rgba ? c->d_rgba : nullptr, labels ? c->d_labels : nullptr, n, freespace, stats);
}

// n_known: the number of valid pixels if the caller has counted them (the host-pointer entry: the image is in host memory
// anyway), else -1: the compacted count is read back from the device before the frame is enqueued.
static int integrate_depth_impl(ks_ctx* c, const float T[7], DepthParams D, int freespace, ks_frame_stats* stats, long long n_known = -1) {
  const size_t n_px = (size_t)D.width * D.height;
  int rc;
  if (n_px > c->cap_points && (rc = quiesce(c))) return rc;  // growing frees buffers a pending tail still needs
  if ((rc = ensure_points(c, n_px))) return rc;
  const uint32_t nb = (uint32_t)((n_px + 1023) / 1024);
  if ((rc = c->d_depth_blocks.reserve(c, (size_t)nb + 1, (size_t)nb + 1))) return rc;
  hipStream_t st = c->stream;
  hipLaunchKernelGGL(k_depth_count, dim3(nb), dim3(1024), 0, st, D, (uint32_t)n_px, c->d_depth_blocks);
  hipLaunchKernelGGL(k_depth_scan, dim3(1), dim3(1024), 0, st, c->d_depth_blocks, nb);
  const bool have_labels = D.label_img != nullptr;
  hipLaunchKernelGGL(k_depth_compact, dim3(nb), dim3(1024), 0, st, D, (uint32_t)n_px, c->d_depth_blocks, c->d_label_lut,
                     c->d_xyz, c->d_rgba, c->d_labels);
  uint32_t n = 0;
  if (n_known >= 0) {
    n = (uint32_t)n_known;   // (the integration order and the sort-key layout depend on n: the host needs it to enqueue the frame)
  } else {
    HIPCHK(c, hipMemcpyAsync(&n, c->d_depth_blocks + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  if (!have_labels && !(D.rgba_img && c->d_color_lut)) {
    c->err = "ks_integrate_depth: need a label image, or a colour image plus ks_set_color_to_label";
    return KS_ERR_INVALID_ARG;
  }
  return integrate_device(c, T, c->d_xyz, c->d_rgba, have_labels ? c->d_labels : nullptr, n, freespace, stats);
}

int ks_integrate_depth(ks_ctx* c, const float T[7], const void* depth, int depth_fmt, const uint8_t* label_img,
                       const uint8_t* rgba_img, int width, int height, const float K[4], int freespace,
                       ks_frame_stats* stats) {
  if (!c || !T || !depth || !K || width <= 0 || height <= 0 || (depth_fmt != 0 && depth_fmt != 1)) return KS_ERR_INVALID_ARG;
  const size_t n_px = (size_t)width * height;
  const size_t dbytes = n_px * (depth_fmt == 0 ? 4 : 2);
  if (int rc = c->d_img_depth.reserve(c, dbytes, dbytes)) return rc;
  if (int rc = c->d_img_aux.reserve(c, n_px * 4, n_px * 4)) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_img_depth, depth, dbytes, hipMemcpyHostToDevice, c->stream));
  DepthParams D{};
  D.depth = c->d_img_depth;
  if (label_img) {
    HIPCHK(c, hipMemcpyAsync(c->d_img_aux, label_img, n_px, hipMemcpyHostToDevice, c->stream));
    D.label_img = c->d_img_aux;
  } else if (rgba_img) {
    HIPCHK(c, hipMemcpyAsync(c->d_img_aux, rgba_img, n_px * 4, hipMemcpyHostToDevice, c->stream));
    D.rgba_img = c->d_img_aux;
  }
  D.fmt = depth_fmt;
  D.width = width;
  D.height = height;
  D.cx = K[2];
  D.cy = K[3];
  // unit_scaling / fx evaluated in double then narrowed, as depth_map_to_pointcloud.h:227-229
  const double unit = depth_fmt == 0 ? 1.0 : 0.001;
  D.constant_x = (float)(unit / (double)K[0]);
  D.constant_y = (float)(unit / (double)K[1]);
  // the valid pixels (ks_k_io.h: depth_pixel — finite f32 / non-zero u16), counted here while the copies are in flight: no
  // read-back of the compacted count, no host wait before the frame is enqueued
  long long n_valid = 0;
  if (depth_fmt == 0) {
    const float* d = (const float*)depth;
    for (size_t i = 0; i < n_px; ++i) n_valid += std::isfinite(d[i]) ? 1 : 0;
  } else {
    const uint16_t* d = (const uint16_t*)depth;
    for (size_t i = 0; i < n_px; ++i) n_valid += d[i] != 0 ? 1 : 0;
  }
  return integrate_depth_impl(c, T, D, freespace, stats, n_valid);
}

int ks_integrate_depth_device(ks_ctx* c, const float T[7], const void* d_depth, int depth_fmt, const uint8_t* d_label_img,
                              const uint8_t* d_rgba_img, int width, int height, const float K[4], int freespace,
                              ks_frame_stats* stats) {
  if (!c || !T || !d_depth || !K || width <= 0 || height <= 0 || (depth_fmt != 0 && depth_fmt != 1)) return KS_ERR_INVALID_ARG;
  DepthParams D{};
  D.depth = d_depth;
  D.label_img = d_label_img;
  D.rgba_img = d_label_img ? nullptr : d_rgba_img;
  D.fmt = depth_fmt;
  D.width = width;
  D.height = height;
  D.cx = K[2];
  D.cy = K[3];
  const double unit = depth_fmt == 0 ? 1.0 : 0.001;
  D.constant_x = (float)(unit / (double)K[0]);
  D.constant_y = (float)(unit / (double)K[1]);
  return integrate_depth_impl(c, T, D, freespace, stats);
}

int ks_num_blocks(ks_ctx* c, size_t* n) { return collect_block_indices(c, false, false, nullptr, 0, n); }
int ks_get_block_indices(ks_ctx* c, int32_t* out, size_t cap, size_t* n) { return collect_block_indices(c, false, false, out, cap, n); }
int ks_get_updated_block_indices(ks_ctx* c, int32_t* out, size_t cap, size_t* n, int reset) { return collect_block_indices(c, true, reset != 0, out, cap, n); }

int ks_download_blocks(ks_ctx* c, const int32_t* idx, size_t n, void* tsdf_out, void* sem_out) {
  if (!c || (n && !idx)) return KS_ERR_INVALID_ARG;
  if (n == 0) return KS_OK;
  if (int rc = quiesce(c)) return rc;
  const int vps = c->cfg.voxels_per_side;
  const size_t nv = (size_t)vps * vps * vps;
  // chunk so staging buffers stay bounded (<= ~256 MiB of semantic voxels)
  const size_t chunk = std::max<size_t>(1, (size_t(256) << 20) / (nv * 92));
  if (c->cap_out_blocks < std::min(chunk, n)) {
    const size_t cb = std::min(chunk, std::max<size_t>(n, 16));
    c->cap_out_blocks = 0;
    int rc;
    if ((rc = c->d_tsdf_out.alloc(c, cb * nv * 12))) return rc;
    if ((rc = c->d_sem_out.alloc(c, cb * nv * 92))) return rc;
    if ((rc = c->d_block_idx.alloc(c, cb * 3))) return rc;
    c->cap_out_blocks = cb;
  }
  for (size_t off = 0; off < n; off += c->cap_out_blocks) {
    const size_t m = std::min(c->cap_out_blocks, n - off);
    HIPCHK(c, hipMemcpyAsync(c->d_block_idx, idx + 3 * off, m * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_download, dim3((uint32_t)((nv + 255) / 256), (uint32_t)m), dim3(256), 0, c->stream, c->table,
                       c->pool, c->d_block_idx, vps, c->d_label_lut, tsdf_out ? c->d_tsdf_out : nullptr,
                       sem_out ? c->d_sem_out : nullptr);
    if (tsdf_out)
      HIPCHK(c, hipMemcpyAsync((uint8_t*)tsdf_out + off * nv * 12, c->d_tsdf_out, m * nv * 12, hipMemcpyDeviceToHost, c->stream));
    if (sem_out)
      HIPCHK(c, hipMemcpyAsync((uint8_t*)sem_out + off * nv * 92, c->d_sem_out, m * nv * 92, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return KS_OK;
}

int ks_upload_blocks(ks_ctx* c, const int32_t* idx, size_t n, const void* tsdf_in, const void* sem_in) {
  if (!c || (n && !idx) || (!tsdf_in && !sem_in)) return KS_ERR_INVALID_ARG;
  if (n == 0) return KS_OK;
  if (c->fatal) return KS_ERR_INVALID_ARG;
  const int vps = c->cfg.voxels_per_side;
  const int tpb = vps / 8;  // tiles per block edge
  const size_t nv = (size_t)vps * vps * vps;
  std::vector<uint64_t> keys;
  keys.reserve(n * tpb * tpb * tpb);
  const int lim = kTileBias / tpb;
  for (size_t b = 0; b < n; ++b) {
    const int bx = idx[3 * b], by = idx[3 * b + 1], bz = idx[3 * b + 2];
    if (bx < -lim || bx >= lim || by < -lim || by >= lim || bz < -lim || bz >= lim) {
      c->err = "block index outside the packed tile-key range";
      return KS_ERR_INDEX_RANGE;
    }
    for (int z = 0; z < tpb; ++z)
      for (int y = 0; y < tpb; ++y)
        for (int x = 0; x < tpb; ++x) keys.push_back(pack_tile(bx * tpb + x, by * tpb + y, bz * tpb + z));
  }
  DevBuf<uint64_t> d_keys;
  int rc;
  if ((rc = d_keys.alloc(c, keys.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(d_keys, keys.data(), keys.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  if ((rc = insert_tiles(c, d_keys, keys.size()))) return rc;   // (synchronises the stream: d_keys may go)
  // staging buffers shared with ks_download_blocks
  const size_t chunk = std::max<size_t>(1, (size_t(256) << 20) / (nv * 92));
  if (c->cap_out_blocks < std::min(chunk, n)) {
    const size_t cb = std::min(chunk, std::max<size_t>(n, 16));
    c->cap_out_blocks = 0;
    if ((rc = c->d_tsdf_out.alloc(c, cb * nv * 12))) return rc;
    if ((rc = c->d_sem_out.alloc(c, cb * nv * 92))) return rc;
    if ((rc = c->d_block_idx.alloc(c, cb * 3))) return rc;
    c->cap_out_blocks = cb;
  }
  for (size_t off = 0; off < n; off += c->cap_out_blocks) {
    const size_t m = std::min(c->cap_out_blocks, n - off);
    HIPCHK(c, hipMemcpyAsync(c->d_block_idx, idx + 3 * off, m * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (tsdf_in)
      HIPCHK(c, hipMemcpyAsync(c->d_tsdf_out, (const uint8_t*)tsdf_in + off * nv * 12, m * nv * 12, hipMemcpyHostToDevice, c->stream));
    if (sem_in)
      HIPCHK(c, hipMemcpyAsync(c->d_sem_out, (const uint8_t*)sem_in + off * nv * 92, m * nv * 92, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_upload, dim3((uint32_t)((nv + 255) / 256), (uint32_t)m), dim3(256), 0, c->stream, c->table, c->pool,
                       c->d_block_idx, vps, tsdf_in ? (const uint8_t*)c->d_tsdf_out : nullptr,
                       sem_in ? (const uint8_t*)c->d_sem_out : nullptr);
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

// ---- semantic mesh (ks_k_mesh.h) -------------------------------------------------------------------------
static int mesh_scratch(ks_ctx* c, int i, size_t bytes) {
  return c->d_mesh_buf[i].reserve(c, bytes, std::max<size_t>(bytes + bytes / 2, 256));
}
static int mesh_arena_reserve(ks_ctx* c, int a, size_t n_vertices) {
  if (n_vertices <= c->mesh_cap[a]) return KS_OK;
  const size_t cap = std::max<size_t>(n_vertices + n_vertices / 2, 4096);
  c->mesh_cap[a] = 0;
  int rc;
  if ((rc = c->mesh_xyz[a].alloc(c, 3 * cap))) return rc;
  if ((rc = c->mesh_nrm[a].alloc(c, 3 * cap))) return rc;
  if ((rc = c->mesh_rgba[a].alloc(c, cap))) return rc;
  if ((rc = c->mesh_label[a].alloc(c, cap))) return rc;
  c->mesh_arena[a] = MeshArena{c->mesh_xyz[a], c->mesh_nrm[a], c->mesh_rgba[a], c->mesh_label[a]};
  c->mesh_cap[a] = cap;
  return KS_OK;
}
static int holds_voxels(ks_ctx* c, const char* who) {
  if (!c->shard_export) return KS_OK;
  c->err = std::string(who) + ": a marcher context of ks_integrate_round_exact holds no voxel data";
  return KS_ERR_UNSUPPORTED;
}
// ks_mesh_changed_blocks, ks_esdf_changed_blocks: the count, and the triples when a buffer is given
static int copy_block_list(ks_ctx* c, const char* who, const std::vector<int32_t>& blocks, int32_t* out_xyz, size_t cap, size_t* n) {
  if (!n) return KS_ERR_INVALID_ARG;
  *n = blocks.size() / 3;
  if (out_xyz) {
    if (cap < *n) {
      c->err = std::string(who) + ": output buffer too small";
      return KS_ERR_INVALID_ARG;
    }
    std::memcpy(out_xyz, blocks.data(), blocks.size() * sizeof(int32_t));
  }
  return KS_OK;
}

// The bookkeeping of a mesh update: pure arithmetic over block words (pack_coord3 of block indices; every vector ascending).
struct MeshPlan {
  std::vector<uint64_t> B, R;        // every block of the map; of them, the blocks to mesh
  std::vector<uint32_t> dir_in;      // per block of B: {its number in R, 0}, or {0xffffffff, the vertices it keeps}
  std::vector<uint32_t> old_first;   // per block of B: where the vertices it keeps are now
};
// blocks, old_dir: the block list so far and the directory of the last update (in the same order); fresh, stale: the blocks of the
// tiles that joined the map, and of those written, since then; full: mesh everything and keep nothing
static MeshPlan mesh_plan(const std::vector<uint64_t>& blocks, const std::vector<ks_mesh_block>& old_dir, const std::vector<uint64_t>& fresh,
                          const std::vector<uint64_t>& stale, bool full) {
  MeshPlan P;
  std::vector<uint64_t>&B = P.B, &R = P.R;
  // 1) the block list grows by the tiles that joined the map
  std::set_union(blocks.begin(), blocks.end(), fresh.begin(), fresh.end(), std::back_inserter(B));
  // 2) what to mesh: everything, or the blocks with a stale tile plus the up to seven blocks at -x / -y / -z offsets whose
  //    border cubes read it
  if (full) {
    R = B;
  } else {
    std::vector<uint64_t> cand;
    for (uint64_t w : stale) {
      int b[3];
      unpack_coord3(w, b[0], b[1], b[2]);
      for (int o = 0; o < 8; ++o) cand.push_back(pack_coord3(b[0] - (o & 1), b[1] - ((o >> 1) & 1), b[2] - (o >> 2)));
    }
    sort_unique(cand);
    std::set_intersection(cand.begin(), cand.end(), B.begin(), B.end(), std::back_inserter(R));
  }
  // 3) the new directory: re-meshed blocks by their number in R, kept ones with the segment they have
  const size_t nb = B.size(), nr = R.size();
  auto old_word = [&](size_t io) { return pack_coord3(old_dir[io].block[0], old_dir[io].block[1], old_dir[io].block[2]); };
  P.dir_in.assign(2 * nb, 0u);
  P.old_first.assign(nb, 0u);
  size_t ir = 0, io = 0;
  for (size_t i = 0; i < nb; ++i) {
    while (ir < nr && R[ir] < B[i]) ++ir;
    if (ir < nr && R[ir] == B[i]) {
      P.dir_in[2 * i] = (uint32_t)ir;
      continue;
    }
    P.dir_in[2 * i] = 0xffffffffu;
    while (io < old_dir.size() && old_word(io) < B[i]) ++io;
    if (!full && io < old_dir.size() && old_word(io) == B[i]) {
      P.dir_in[2 * i + 1] = old_dir[io].n_vertices;
      P.old_first[i] = old_dir[io].first_vertex;
    }
  }
  return P;
}

int ks_mesh_default_config(ks_mesh_config* m) {
  if (!m) return KS_ERR_INVALID_ARG;
  m->min_weight = 1e-4f;
  m->only_stale = 0;
  return KS_OK;
}

int ks_mesh_update(ks_ctx* c, const ks_mesh_config* m, ks_mesh_stats* stats) {
  if (!c || !m) return KS_ERR_INVALID_ARG;
  c->mi_valid = false;   // the indexed view is a snapshot of the mesh this call replaces (rule 7)
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!(m->min_weight > 0.0f) || !std::isfinite(m->min_weight)) {
    c->err = "ks_mesh_update: min_weight must be a finite positive number";
    return KS_ERR_INVALID_ARG;
  }
  if (int rc = holds_voxels(c, "ks_mesh_update")) return rc;
  if (int rc = quiesce(c)) return rc;
  hipStream_t st = c->stream;
  const int sh = c->vps_shift;
  int rc;
  // the stale flags, the tiles that joined the map since the last call, and what follows from them (mesh_plan)
  TileSnapshot snap(c);
  const uint32_t nt = snap.nt;
  if ((rc = snap.fetch_flags(c, c->pool.mesh_stale()))) return rc;
  if (nt) hipLaunchKernelGGL(k_stale_clear, dim3((nt + 255) / 256), dim3(256), 0, st, c->pool.mesh_stale(), nt, kStaleMesh);   // (the ESDF's bit stays)
  std::vector<uint64_t> fresh, stale;   // blocks of the tiles that joined the map since the last call, and of the stale ones
  if ((rc = snap.blocks(c, sh, c->mesh_tiles_seen, 0, &fresh))) return rc;
  const bool full = !m->only_stale || !c->mesh_valid || m->min_weight != c->mesh_min_weight;
  c->mesh_valid = false;   // (a failure below leaves flags cleared that nothing has meshed: the next call starts over)
  if (!full && (rc = snap.blocks(c, sh, 0, kStaleMesh, &stale))) return rc;
  // a block that left the map since the last update carries no flag: it counts as written, so that the resident blocks whose
  // border cubes read it are re-meshed (it is no block of the map itself: mesh_plan keeps the blocks of the list only)
  const std::vector<uint64_t> removed = std::move(c->mesh_removed);
  c->mesh_removed.clear();
  if (!full && !removed.empty()) {
    std::vector<uint64_t> both;
    std::set_union(stale.begin(), stale.end(), removed.begin(), removed.end(), std::back_inserter(both));
    stale.swap(both);
  }
  MeshPlan P = mesh_plan(c->mesh_blocks, c->mesh_dir, fresh, stale, full);
  c->mesh_blocks.swap(P.B);
  c->mesh_tiles_seen = nt;
  const std::vector<uint64_t>& B = c->mesh_blocks;
  const std::vector<uint32_t>&dir_in = P.dir_in, &old_first = P.old_first;
  const size_t nb = B.size(), nr = P.R.size();
  std::vector<ks_mesh_block> dir(nb);
  for (size_t i = 0; i < nb; ++i) unpack_coord3(B[i], dir[i].block[0], dir[i].block[1], dir[i].block[2]);
  std::vector<int32_t> r_triples;   // the blocks to mesh, as the kernels take them
  words_to_triples(P.R, &r_triples);
  {
    // what this update replaces: the segments of the re-meshed blocks, and those of the blocks that left the map
    std::vector<uint64_t> changed;
    std::set_union(P.R.begin(), P.R.end(), removed.begin(), removed.end(), std::back_inserter(changed));
    words_to_triples(changed, &c->mesh_changed);
  }
  unsigned long long degenerate = 0;
  uint32_t total = 0;
  const int from = c->mesh_cur, to = c->mesh_cur ^ 1;
  if (nb) {
    const size_t nvb = (size_t)512 << (3 * sh);
    const uint32_t tiles_per_block = 1u << (3 * sh);
    if (nr * (size_t)tiles_per_block >= (1ull << 31) || nr * nvb * 5 >= (1ull << 36)) {
      c->err = "ks_mesh_update: too many blocks for one call";
      return KS_ERR_INVALID_ARG;
    }
    if ((rc = mesh_scratch(c, 0, std::max<size_t>(nr, 1) * 12)) || (rc = mesh_scratch(c, 1, std::max<size_t>(nr, 1) * nvb)) ||
        (rc = mesh_scratch(c, 2, std::max<size_t>(nr, 1) * nvb * 4)) || (rc = mesh_scratch(c, 3, std::max<size_t>(nr, 1) * 4)) ||
        (rc = mesh_scratch(c, 4, std::max<size_t>(nr, 1) * 4)) || (rc = mesh_scratch(c, 5, nb * 8)) || (rc = mesh_scratch(c, 6, (nb + 1) * 4)) ||
        (rc = mesh_scratch(c, 7, nb * 4)) || (rc = mesh_scratch(c, 8, nb * 12)) || (rc = mesh_scratch(c, 9, 8)))
      return rc;
    MeshWork W{};
    W.rblocks = (const int32_t*)c->d_mesh_buf[0].get();
    W.cube_cnt = c->d_mesh_buf[1];
    W.cube_off = (uint32_t*)c->d_mesh_buf[2].get();
    W.block_tri = (uint32_t*)c->d_mesh_buf[3].get();
    W.rb_first = (uint32_t*)c->d_mesh_buf[4].get();
    W.degenerate = (unsigned long long*)c->d_mesh_buf[9].get();
    W.voxel_size = c->cfg.voxel_size;
    W.min_weight = m->min_weight;
    W.vps_shift = sh;
    uint32_t* d_dir_out = (uint32_t*)c->d_mesh_buf[6].get();
    HIPCHK(c, hipMemsetAsync(W.degenerate, 0, 8, st));
    HIPCHK(c, hipMemcpyAsync(c->d_mesh_buf[5], dir_in.data(), nb * 8, hipMemcpyHostToDevice, st));
    if (nr) {
      HIPCHK(c, hipMemcpyAsync(c->d_mesh_buf[0], r_triples.data(), nr * 12, hipMemcpyHostToDevice, st));
      HIPCHK(c, hipMemsetAsync(W.cube_cnt, 0, nr * nvb, st));
      hipLaunchKernelGGL(k_mesh_tiles<false>, dim3((uint32_t)(nr * tiles_per_block)), dim3(512), 0, st, c->table, c->pool, W, MeshArena{});
      hipLaunchKernelGGL(k_mesh_scan, dim3((uint32_t)nr), dim3(1024), 0, st, W);
    }
    hipLaunchKernelGGL(k_mesh_dir, dim3(1), dim3(1024), 0, st, W, (const uint2*)c->d_mesh_buf[5].get(), (uint32_t)nb, d_dir_out, (uint32_t*)c->d_mesh_buf[7].get());
    std::vector<uint32_t> first(nb + 1);
    HIPCHK(c, hipMemcpyAsync(first.data(), d_dir_out, (nb + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&degenerate, W.degenerate, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    total = first[nb];
    if ((rc = mesh_arena_reserve(c, to, total))) return rc;
    std::vector<uint32_t> moves;
    for (size_t i = 0; i < nb; ++i) {
      dir[i].first_vertex = first[i];
      dir[i].n_vertices = first[i + 1] - first[i];
      if (dir_in[2 * i] == 0xffffffffu && dir[i].n_vertices) {
        moves.push_back(old_first[i]);
        moves.push_back(first[i]);
        moves.push_back(dir[i].n_vertices);
      }
    }
    if (nr && total) hipLaunchKernelGGL(k_mesh_tiles<true>, dim3((uint32_t)(nr * tiles_per_block)), dim3(512), 0, st, c->table, c->pool, W, c->mesh_arena[to]);
    if (!moves.empty()) {
      HIPCHK(c, hipMemcpyAsync(c->d_mesh_buf[8], moves.data(), moves.size() * 4, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_mesh_copy, dim3((uint32_t)(moves.size() / 3)), dim3(256), 0, st, c->mesh_arena[from], c->mesh_arena[to], (const uint32_t*)c->d_mesh_buf[8].get());
    }
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
  } else if (nt) {
    HIPCHK(c, hipStreamSynchronize(st));
  }
  c->mesh_cur = to;
  c->mesh_dir.swap(dir);
  c->mesh_valid = true;
  c->mesh_min_weight = m->min_weight;
  if (stats) {
    stats->blocks_meshed = nr;
    stats->blocks_total = nb;
    stats->triangles_total = total / 3;
    stats->degenerate_dropped = degenerate;
    uint64_t ch = 0;
    for (size_t i = 0; i < nb; ++i)
      if (dir_in[2 * i] != 0xffffffffu) ch += c->mesh_dir[i].n_vertices / 3;
    stats->triangles_changed = ch;
  }
  return KS_OK;
}

int ks_mesh_size(ks_ctx* c, size_t* n_blocks, size_t* n_vertices) {
  if (!c) return KS_ERR_INVALID_ARG;
  size_t b = 0, v = 0;
  for (const ks_mesh_block& d : c->mesh_dir) {
    b += d.n_vertices != 0;
    v += d.n_vertices;
  }
  if (n_blocks) *n_blocks = b;
  if (n_vertices) *n_vertices = v;
  return KS_OK;
}

int ks_mesh_download(ks_ctx* c, ks_mesh_block* blocks, size_t cap_blocks, float* xyz, float* normals, uint8_t* rgba, uint8_t* labels,
                     size_t cap_vertices) {
  if (!c) return KS_ERR_INVALID_ARG;
  size_t nbl = 0, nv = 0;
  ks_mesh_size(c, &nbl, &nv);
  if ((blocks && cap_blocks < nbl) || ((xyz || normals || rgba || labels) && cap_vertices < nv)) {
    c->err = "ks_mesh_download: output buffer too small (call ks_mesh_size first)";
    return KS_ERR_INVALID_ARG;
  }
  if (blocks) {
    size_t o = 0;
    for (const ks_mesh_block& d : c->mesh_dir)
      if (d.n_vertices) blocks[o++] = d;
  }
  if (nv == 0) return KS_OK;
  const MeshArena& A = c->mesh_arena[c->mesh_cur];
  hipStream_t st = c->stream;
  if (xyz) HIPCHK(c, hipMemcpyAsync(xyz, A.xyz, nv * 12, hipMemcpyDeviceToHost, st));
  if (normals) HIPCHK(c, hipMemcpyAsync(normals, A.nrm, nv * 12, hipMemcpyDeviceToHost, st));
  if (rgba) HIPCHK(c, hipMemcpyAsync(rgba, A.rgba, nv * 4, hipMemcpyDeviceToHost, st));
  if (labels) HIPCHK(c, hipMemcpyAsync(labels, A.label, nv, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return KS_OK;
}

int ks_mesh_changed_blocks(ks_ctx* c, int32_t* out_xyz, size_t cap, size_t* n) {
  return c ? copy_block_list(c, "ks_mesh_changed_blocks", c->mesh_changed, out_xyz, cap, n) : KS_ERR_INVALID_ARG;
}

// ---- indexed view of the stored mesh (ks_k_mesh_index.h) ------------------------------------
// inclusive scan of n words in place; the total -> *total
static void mi_scan(ks_ctx* c, uint32_t* v, uint32_t n, uint32_t* total) {
  const uint32_t nb = (n + kMiSlice - 1) / kMiSlice;
  hipLaunchKernelGGL(k_mi_scan_partial, dim3(nb), dim3(256), 0, c->stream, (const uint32_t*)v, n, c->mi_partial.get());
  hipLaunchKernelGGL(k_mi_scan_top, dim3(1), dim3(1024), 0, c->stream, c->mi_partial.get(), nb, total);
  hipLaunchKernelGGL(k_mi_scan_apply, dim3(nb), dim3(256), 0, c->stream, v, n, (const uint32_t*)c->mi_partial.get());
}
static int mesh_index_ready(ks_ctx* c, const char* who) {
  if (int rc = holds_voxels(c, who)) return rc;
  if (c->fatal) {
    c->err = std::string(who) + ": context is in a failed state (earlier pool/index error)";
    return KS_ERR_INVALID_ARG;
  }
  if (c->mi_valid) return KS_OK;
  c->err = std::string(who) + ": no index is stored (ks_mesh_index has not run since the last ks_mesh_update or clear)";
  return KS_ERR_INVALID_ARG;
}

int ks_mesh_index(ks_ctx* c, ks_mesh_index_stats* stats) {
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!c) return KS_ERR_INVALID_ARG;
  if (int rc = holds_voxels(c, "ks_mesh_index")) return rc;
  if (c->fatal) {
    c->err = "ks_mesh_index: context is in a failed state (earlier pool/index error)";
    return KS_ERR_INVALID_ARG;
  }
  if (int rc = quiesce(c)) return rc;   // (the frames in flight; their statistics stay owed)
  if (!c->mesh_valid) {
    c->err = "ks_mesh_index: no mesh is stored (ks_mesh_update has not succeeded since the map was created or cleared)";
    return KS_ERR_INVALID_ARG;
  }
  c->mi_valid = false;   // (a failure below leaves no index)
  size_t nc = 0;
  ks_mesh_size(c, nullptr, &nc);
  if (nc >= ((size_t)1 << 31)) {
    c->err = "ks_mesh_index: too many corners for one call";
    return KS_ERR_UNSUPPORTED;
  }
  uint32_t counts[2] = {0, 0};
  uint64_t workspace = 0;
  if (nc) {
    const uint32_t n = (uint32_t)nc;
    const size_t cap = std::max<size_t>(nc + nc / 2, 256), nb = (nc + kMiSlice - 1) / kMiSlice;
    int rc;
    for (int k = 0; k < 2; ++k)
      if ((rc = c->mi_key32[k].reserve(c, nc, cap)) || (rc = c->mi_val[k].reserve(c, nc, cap)) || (rc = c->mi_key64[k].reserve(c, nc, cap))) return rc;
    if ((rc = c->mi_partial.reserve(c, nb, nb + nb / 2 + 16)) || (rc = c->mi_counts.reserve(c, 4, 4)) || (rc = c->mi_xyz.reserve(c, 3 * nc, 3 * cap)) ||
        (rc = c->mi_nrm.reserve(c, 3 * nc, 3 * cap)) || (rc = c->mi_rgba.reserve(c, nc, cap)) || (rc = c->mi_obj.reserve(c, nc, cap)) ||
        (rc = c->mi_valence.reserve(c, nc, cap)) || (rc = c->mi_label.reserve(c, nc, cap)) || (rc = c->mi_indices.reserve(c, nc, cap)))
      return rc;
    workspace = (uint64_t)nc * (2 * 4 + 2 * 4 + 2 * 8 + 12 + 12 + 4 + 4 + 4 + 1 + 4) + (uint64_t)nb * 4 + 16;
    hipStream_t st = c->stream;
    const MeshArena& A = c->mesh_arena[c->mesh_cur];
    const dim3 per_corner((n + 255u) / 256u);
    // 1) the corners grouped by position: stable sorts on the bits of z, then of (x, y)
    hipLaunchKernelGGL(k_mi_keys_z, per_corner, dim3(256), 0, st, (const float*)A.xyz, n, c->mi_key32[0].get(), c->mi_val[0].get());
    uint32_t* k32 = nullptr;
    uint32_t* perm = nullptr;
    if ((rc = sort_pairs(c, c->mi_key32[0].get(), c->mi_key32[1].get(), c->mi_val[0].get(), c->mi_val[1].get(), nc, 32, &k32, &perm))) return rc;
    hipLaunchKernelGGL(k_mi_keys_xy, per_corner, dim3(256), 0, st, (const float*)A.xyz, (const uint32_t*)perm, n, c->mi_key64[0].get());
    uint64_t* k64 = nullptr;
    uint32_t* other = perm == c->mi_val[0].get() ? c->mi_val[1].get() : c->mi_val[0].get();
    if ((rc = sort_pairs(c, c->mi_key64[0].get(), c->mi_key64[1].get(), perm, other, nc, 64, &k64, &perm))) return rc;
    // (the 32-bit key buffers and the payload buffer the result is not in are free from here on)
    uint32_t* run = c->mi_key32[0].get();
    uint32_t* vertex_of = c->mi_key32[1].get();
    uint32_t* first_corner = perm == c->mi_val[0].get() ? c->mi_val[1].get() : c->mi_val[0].get();
    uint32_t* d_counts = c->mi_counts.get();
    HIPCHK(c, hipMemsetAsync(d_counts, 0, 16, st));
    HIPCHK(c, hipMemsetAsync(vertex_of, 0, nc * 4, st));
    HIPCHK(c, hipMemsetAsync(c->mi_nrm, 0, nc * 12, st));
    HIPCHK(c, hipMemsetAsync(c->mi_valence, 0, nc * 4, st));
    // 2) runs of equal positions, their first corners, the vertex numbers in corner order
    hipLaunchKernelGGL(k_mi_heads, per_corner, dim3(256), 0, st, (const float*)A.xyz, (const uint32_t*)perm, n, run);
    mi_scan(c, run, n, d_counts + 2);
    hipLaunchKernelGGL(k_mi_first, per_corner, dim3(256), 0, st, (const uint32_t*)perm, (const uint32_t*)run, n, first_corner, vertex_of);
    mi_scan(c, vertex_of, n, d_counts);
    // 3) indices, attributes, normal sums; normals
    MeshIndexOut O{c->mi_xyz, c->mi_nrm, c->mi_rgba, c->mi_label, c->mi_indices, c->mi_valence};
    hipLaunchKernelGGL(k_mi_emit, per_corner, dim3(256), 0, st, A, (const uint32_t*)perm, (const uint32_t*)run, (const uint32_t*)first_corner,
                       (const uint32_t*)vertex_of, n, O);
    hipLaunchKernelGGL(k_mi_finish, per_corner, dim3(256), 0, st, O, d_counts);
    HIPCHK(c, hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));   // the one read-back: vertices, largest valence
    // 4) the object of every vertex, as ks_objects_query answers for its position
    if (c->obj_valid) {
      hipLaunchKernelGGL(k_obj_query, dim3((counts[0] + 255u) / 256u), dim3(256), 0, st, c->table, (const uint32_t*)c->obj_ids.get(), c->obj_tiles,
                         (const float*)c->mi_xyz.get(), (size_t)counts[0], c->voxel_size_inv, c->mi_obj.get());
    } else {
      HIPCHK(c, hipMemsetAsync(c->mi_obj, 0xff, (size_t)counts[0] * 4, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
  }
  c->mi_corners = nc;
  c->mi_vertices = counts[0];
  c->mi_valid = true;
  if (stats) {
    stats->corners = nc;
    stats->vertices = counts[0];
    stats->max_corners_per_vertex = counts[1];
    stats->workspace_bytes = workspace;
  }
  return KS_OK;
}

int ks_mesh_index_size(ks_ctx* c, size_t* n_vertices, size_t* n_indices) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (int rc = mesh_index_ready(c, "ks_mesh_index_size")) return rc;
  if (n_vertices) *n_vertices = c->mi_vertices;
  if (n_indices) *n_indices = c->mi_corners;
  return KS_OK;
}

int ks_mesh_index_download(ks_ctx* c, float* xyz, float* normals, uint8_t* rgba, uint8_t* labels, uint32_t* object_ids, size_t cap_vertices,
                           uint32_t* indices, size_t cap_indices) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (int rc = mesh_index_ready(c, "ks_mesh_index_download")) return rc;
  const size_t nv = c->mi_vertices, nc = c->mi_corners;
  if (((xyz || normals || rgba || labels || object_ids) && cap_vertices < nv) || (indices && cap_indices < nc)) {
    c->err = "ks_mesh_index_download: output buffer too small (call ks_mesh_index_size first)";
    return KS_ERR_INVALID_ARG;
  }
  if (nc == 0) return KS_OK;
  hipStream_t st = c->stream;
  if (xyz) HIPCHK(c, hipMemcpyAsync(xyz, c->mi_xyz, nv * 12, hipMemcpyDeviceToHost, st));
  if (normals) HIPCHK(c, hipMemcpyAsync(normals, c->mi_nrm, nv * 12, hipMemcpyDeviceToHost, st));
  if (rgba) HIPCHK(c, hipMemcpyAsync(rgba, c->mi_rgba, nv * 4, hipMemcpyDeviceToHost, st));
  if (labels) HIPCHK(c, hipMemcpyAsync(labels, c->mi_label, nv, hipMemcpyDeviceToHost, st));
  if (object_ids) HIPCHK(c, hipMemcpyAsync(object_ids, c->mi_obj, nv * 4, hipMemcpyDeviceToHost, st));
  if (indices) HIPCHK(c, hipMemcpyAsync(indices, c->mi_indices, nc * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return KS_OK;
}

// ---- batch ESDF (ks_k_esdf.h) ----------------------------------------------------------------------------
int ks_esdf_default_config(ks_esdf_config* e) {
  if (!e) return KS_ERR_INVALID_ARG;
  std::memset(e, 0, sizeof(*e));
  e->min_weight = 1e-6f;        // Voxblox's EsdfIntegrator::Config
  e->min_distance_m = 0.2f;
  e->max_distance_m = 2.0f;
  e->max_workspace_bytes = 8ull << 30;
  return KS_OK;
}

// The dense box of a batch update: pure arithmetic over the tile directory.
struct EsdfBoxPlan {
  int lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1};   // tiles [lo, hi] of the box
  int r0[3], r1[3];                              // voxels [r0, r1) that get results, counted from the box's corner
  uint64_t nbt[3] = {0, 0, 0};                   // tiles of the box along each axis; all 0: nothing to compute
  uint64_t tiles() const { return nbt[0] * nbt[1] * nbt[2]; }
  // the dense slot grid of the box: the pool slot of each of its tiles, 0xffffffff where none is resident
  std::vector<uint32_t> slot_grid(const TileSnapshot& snap) const {
    std::vector<uint32_t> grid(tiles(), 0xffffffffu);
    for (uint32_t s = 0; s < snap.nt; ++s) {
      int t[3];
      snap.tile(s, t);
      if (t[0] < lo[0] || t[0] > hi[0] || t[1] < lo[1] || t[1] > hi[1] || t[2] < lo[2] || t[2] > hi[2]) continue;
      grid[((size_t)(t[2] - lo[2]) * nbt[1] + (size_t)(t[1] - lo[1])) * nbt[0] + (size_t)(t[0] - lo[0])] = s;
    }
    return grid;
  }
};
// the bounding box of the resident tiles, in tiles; with a region: its tiles dilated by ceil(R / 8), clipped to that box.
// tpb: tiles per block side; R: the reach in voxels
static EsdfBoxPlan esdf_box_plan(const TileSnapshot& snap, const ks_esdf_config& e, int tpb, int R) {
  EsdfBoxPlan P;
  const uint32_t nt = snap.nt;
  for (uint32_t s = 0; s < nt; ++s) {
    int t[3];
    snap.tile(s, t);
    for (int a = 0; a < 3; ++a) {
      if (s == 0 || t[a] < P.lo[a]) P.lo[a] = t[a];
      if (s == 0 || t[a] > P.hi[a]) P.hi[a] = t[a];
    }
  }
  bool empty = nt == 0;
  for (int a = 0; a < 3; ++a) {
    int64_t r0 = (int64_t)P.lo[a] * 8, r1 = ((int64_t)P.hi[a] + 1) * 8;   // voxels [r0, r1) that get results, in world voxel indices
    if (e.use_region && nt) {
      const int64_t t0 = (int64_t)e.region_min[a] * tpb, t1 = ((int64_t)e.region_max[a] + 1) * tpb - 1, grow = (R + 7) / 8;   // tiles [t0, t1]
      r0 = std::max<int64_t>(r0, t0 * 8);
      r1 = std::min<int64_t>(r1, (t1 + 1) * 8);
      P.lo[a] = (int)std::max<int64_t>(P.lo[a], t0 - grow);
      P.hi[a] = (int)std::min<int64_t>(P.hi[a], t1 + grow);
    }
    empty = empty || P.hi[a] < P.lo[a] || r1 <= r0;
    P.r0[a] = (int)std::max<int64_t>(r0 - (int64_t)P.lo[a] * 8, 0);
    P.r1[a] = (int)std::min<int64_t>(r1 - (int64_t)P.lo[a] * 8, ((int64_t)P.hi[a] - P.lo[a] + 1) * 8);
  }
  for (int a = 0; a < 3 && !empty; ++a) P.nbt[a] = (uint64_t)(P.hi[a] - P.lo[a] + 1);
  return P;
}

int ks_esdf_update(ks_ctx* c, const ks_esdf_config* e, ks_esdf_stats* stats) {
  if (!c || !e) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  auto positive = [](float v) { return v > 0.0f && std::isfinite(v); };
  if (!positive(e->min_weight) || !positive(e->min_distance_m) || !positive(e->max_distance_m)) {
    c->err = "ks_esdf_update: min_weight, min_distance_m and max_distance_m must be finite positive numbers";
    return KS_ERR_INVALID_ARG;
  }
  const float reach = ceilf(e->max_distance_m / c->cfg.voxel_size);
  if (!(reach <= (float)kEsdfMaxR)) {
    c->err = "ks_esdf_update: max_distance_m reaches further than 255 voxels";
    return KS_ERR_INVALID_ARG;
  }
  const int R = (int)reach;
  if (e->use_region)
    for (int a = 0; a < 3; ++a)
      if (e->region_min[a] > e->region_max[a]) {
        c->err = "ks_esdf_update: region_min exceeds region_max";
        return KS_ERR_INVALID_ARG;
      }
  if (int rc = holds_voxels(c, "ks_esdf_update")) return rc;
  if (int rc = quiesce(c)) return rc;
  hipStream_t st = c->stream;
  int rc;
  // 1) the box
  TileSnapshot snap(c);
  const uint32_t nt = snap.nt;
  if ((rc = snap.fetch_keys(c))) return rc;
  const EsdfBoxPlan P = esdf_box_plan(snap, *e, c->cfg.voxels_per_side / 8, R);
  const uint64_t* nbt = P.nbt;
  const uint64_t box_tiles = P.tiles(), box_voxels = box_tiles * 512;
  const uint64_t workspace = box_voxels * 32 + box_tiles * 4;   // two key buffers of two planes of 8 bytes; the slot grid
  if (stats) {
    for (int a = 0; a < 3; ++a) stats->box_voxels[a] = nbt[a] * 8;
    stats->workspace_bytes = workspace;
  }
  if (workspace > e->max_workspace_bytes) {
    c->err = "ks_esdf_update: the dense box of " + std::to_string(nbt[0] * 8) + " x " + std::to_string(nbt[1] * 8) + " x " +
             std::to_string(nbt[2] * 8) + " voxels needs " + std::to_string(workspace) + " bytes of work space, more than max_workspace_bytes = " +
             std::to_string(e->max_workspace_bytes) + ": raise it, or compute part of the map with use_region";
    return KS_ERR_UNSUPPORTED;
  }
  if (nbt[0] * 8 >= (1ull << 20) || nbt[1] * 8 >= 65536ull || nbt[2] * 8 >= 65536ull) {   // launch grid limits, far beyond any work space
    c->err = "ks_esdf_update: the box is too large for one call; use use_region";
    return KS_ERR_UNSUPPORTED;
  }
  // 2) the store: default records for every resident tile
  c->esdf_valid = false;   // (a failure below leaves no half-written snapshot readable)
  c->nav_valid = false;    // the navigation field is a snapshot of the store this call replaces
  drop_frontiers(c);       // ... and so are the frontiers (§21)
  drop_rooms(c);           // ... and the rooms (§25)
  if ((rc = c->esdf_store.reserve(c, (size_t)nt * kTileVoxels, ((size_t)nt + nt / 2 + 64) * kTileVoxels))) return rc;
  if ((rc = c->esdf_counters.reserve(c, 3, 3))) return rc;
  HIPCHK(c, hipMemsetAsync(c->esdf_counters, 0, 3 * sizeof(unsigned long long), st));
  if (nt)
    hipLaunchKernelGGL(k_esdf_fill, dim3((uint32_t)(((size_t)nt * kTileVoxels + 255) / 256)), dim3(256), 0, st, c->esdf_store.get(),
                       (size_t)nt * kTileVoxels);
  unsigned long long counts[3] = {0, 0, 0};
  if (box_tiles) {
    // 3) the dense slot grid of the box
    const std::vector<uint32_t> grid = P.slot_grid(snap);
    if ((rc = c->esdf_slots.reserve(c, box_tiles, box_tiles + box_tiles / 2))) return rc;
    for (auto& K : c->esdf_keys)
      if ((rc = K.reserve(c, 2 * box_voxels, 2 * box_voxels + box_voxels / 2))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->esdf_slots, grid.data(), box_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    EsdfBox B{};
    B.nx = (int)(nbt[0] * 8);
    B.ny = (int)(nbt[1] * 8);
    B.nz = (int)(nbt[2] * 8);
    std::copy(P.r0, P.r0 + 3, B.r0);
    std::copy(P.r1, P.r1 + 3, B.r1);
    B.R = R;
    B.voxel_size = c->cfg.voxel_size;
    B.min_weight = e->min_weight;
    B.min_distance = e->min_distance_m;
    B.max_distance = e->max_distance_m;
    B.slots = c->esdf_slots;
    const uint32_t along = 16 * kEsdfPer;
    hipLaunchKernelGGL(k_esdf_x, dim3((uint32_t)((B.nx + 63) / 64), (uint32_t)((B.ny + 3) / 4), (uint32_t)B.nz), dim3(256), 0, st, B, c->pool,
                       c->esdf_keys[0].get());
    hipLaunchKernelGGL(k_esdf_axis<0>, dim3((uint32_t)((B.nx + 15) / 16), (uint32_t)((B.ny + along - 1) / along), (uint32_t)B.nz), dim3(256), 0, st,
                       B, c->pool, (const uint64_t*)c->esdf_keys[0].get(), c->esdf_keys[1].get(), (EsdfRecord*)nullptr,
                       (unsigned long long*)nullptr);
    hipLaunchKernelGGL(k_esdf_axis<1>, dim3((uint32_t)((B.nx + 15) / 16), (uint32_t)((B.nz + along - 1) / along), (uint32_t)B.ny), dim3(256), 0, st,
                       B, c->pool, (const uint64_t*)c->esdf_keys[1].get(), (uint64_t*)nullptr, c->esdf_store.get(), c->esdf_counters.get());
    HIPCHK(c, hipMemcpyAsync(counts, c->esdf_counters, sizeof(counts), hipMemcpyDeviceToHost, st));
  }
  // the snapshot is current everywhere: no tile is stale for ks_esdf_refresh
  if (nt) hipLaunchKernelGGL(k_stale_clear, dim3((nt + 255) / 256), dim3(256), 0, st, c->pool.mesh_stale(), nt, kStaleEsdf);
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  c->esdf_valid = true;
  c->esdf_tiles = nt;
  c->esdf_removed.clear();
  c->esdf_cfg = *e;
  for (int k = 0; k < 3; ++k) c->esdf_totals[k] = counts[k];
  c->esdf_changed.clear();
  if (stats) {
    stats->voxels_observed = counts[0];
    stats->voxels_fixed = counts[1];
    stats->voxels_clamped = counts[2];
  }
  return KS_OK;
}

static int esdf_ready(ks_ctx* c, const char* who) {
  if (c->esdf_valid) return KS_OK;
  c->err = std::string(who) + ": no ESDF is stored (ks_esdf_update has not run since the map was created or cleared)";
  return KS_ERR_INVALID_ARG;
}

// ---- incremental refresh of the stored ESDF ("ESDF", incremental refresh) ----
// The lists of a refresh: pure arithmetic over tile positions (pack_coord3 of tile coordinates; every vector ascending).
struct EsdfLists {
  std::vector<uint64_t> X, Y, Z;   // positions of passes x, y and z; Z = A, the tiles that are recomputed
  std::vector<uint32_t> z_slots;   // pool slot of each tile of Z
  uint64_t n_stale = 0;            // |S|
};
// every position within g of a listed one along `axis`
static std::vector<uint64_t> esdf_dilate(const std::vector<uint64_t>& in, int axis, int g) {
  std::vector<uint64_t> out;
  out.reserve(in.size() * (size_t)(2 * g + 1));
  for (uint64_t p : in)
    for (int d = -g; d <= g; ++d) out.push_back(coord3_moved(p, axis, d));
  sort_unique(out);
  return out;
}
// the positions of `in` that have one of `have` (ascending) within g along `axis`
static std::vector<uint64_t> esdf_keep_near(const std::vector<uint64_t>& in, const std::vector<uint64_t>& have, int axis, int g) {
  std::vector<uint64_t> out;
  for (uint64_t p : in) {
    bool near = false;
    for (int d = -g; d <= g && !near; ++d) near = std::binary_search(have.begin(), have.end(), coord3_moved(p, axis, d));
    if (near) out.push_back(p);
  }
  return out;
}
// keys: slot -> packed tile key; stale: slot -> stale for the ESDF; region: tiles [lo, hi] per axis that hold results.
//   S = the stale tiles;  Z = A = the resident tiles of the region within g of S on every axis;
//   Y = A dilated by g along z, X = Y dilated by g along y — less the positions whose brick can hold no real key: a brick of X
//   has one only with a resident tile within g along x, a brick of Y only with a kept position of X within g along y.  A dropped
//   brick would hold kEsdfNone throughout, which is what a miss reads as.
// removed: the positions of the tiles that left the map since the store was last current (ascending) — stale positions that hold
//   no tile: their sites are gone, so they enter S for the reach (and a position that holds a tile again is in S anyway); n_stale
//   counts resident tiles only.
static void esdf_refresh_lists(const std::vector<uint64_t>& keys, const std::vector<uint8_t>& stale, const std::vector<uint64_t>& removed, int g,
                               bool use_region, const int64_t region_lo[3], const int64_t region_hi[3], EsdfLists* L) {
  const size_t nt = keys.size();
  std::vector<std::pair<uint64_t, uint32_t>> resident(nt);
  std::vector<uint64_t> S;
  for (size_t s = 0; s < nt; ++s) {
    int t[3];
    unpack_tile(keys[s], t[0], t[1], t[2]);
    const uint64_t p = pack_coord3(t[0], t[1], t[2]);
    resident[s] = {p, (uint32_t)s};
    if (stale[s]) S.push_back(p);
  }
  std::sort(resident.begin(), resident.end());
  L->n_stale = S.size();
  S.insert(S.end(), removed.begin(), removed.end());
  sort_unique(S);
  const std::vector<uint64_t> reach = esdf_dilate(esdf_dilate(esdf_dilate(S, 0, g), 1, g), 2, g);
  std::vector<uint64_t> all(nt);
  for (size_t i = 0; i < nt; ++i) {
    all[i] = resident[i].first;
    int t[3];
    unpack_coord3(all[i], t[0], t[1], t[2]);
    bool in = std::binary_search(reach.begin(), reach.end(), all[i]);
    for (int a = 0; a < 3 && in && use_region; ++a) in = t[a] >= region_lo[a] && t[a] <= region_hi[a];
    if (!in) continue;
    L->Z.push_back(all[i]);
    L->z_slots.push_back(resident[i].second);
  }
  const std::vector<uint64_t> y_all = esdf_dilate(L->Z, 2, g);
  L->X = esdf_keep_near(esdf_dilate(y_all, 1, g), all, 0, g);
  L->Y = esdf_keep_near(y_all, L->X, 1, g);
}

int ks_esdf_refresh(ks_ctx* c, uint64_t max_workspace_bytes, ks_esdf_refresh_stats* stats) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (int rc = holds_voxels(c, "ks_esdf_refresh")) return rc;
  if (int rc = esdf_ready(c, "ks_esdf_refresh")) return rc;
  if (int rc = quiesce(c)) return rc;
  hipStream_t st = c->stream;
  const ks_esdf_config& e = c->esdf_cfg;
  if (max_workspace_bytes == 0) max_workspace_bytes = e.max_workspace_bytes;
  const uint32_t nt = c->tiles_initialised, nt_old = c->esdf_tiles;
  const int R = (int)ceilf(e.max_distance_m / c->cfg.voxel_size), g = (R + 7) / 8;
  int rc;
  // 1) the stale tiles (a tile that joined the map since has no records yet: stale whatever its mark says) and the lists
  TileSnapshot snap(c);
  if ((rc = snap.fetch_keys(c)) || (rc = snap.fetch_flags(c, c->pool.mesh_stale()))) return rc;
  for (uint32_t s = 0; s < nt; ++s) snap.flags[s] = (snap.flags[s] & kStaleEsdf) || s >= nt_old;
  int64_t region_lo[3] = {0, 0, 0}, region_hi[3] = {0, 0, 0};
  const int tpb = c->cfg.voxels_per_side / 8;
  for (int a = 0; a < 3; ++a) {
    region_lo[a] = (int64_t)e.region_min[a] * tpb;
    region_hi[a] = ((int64_t)e.region_max[a] + 1) * tpb - 1;
  }
  EsdfLists L;
  const bool tiles_left = !c->esdf_removed.empty();   // a removal since the store was last current
  esdf_refresh_lists(snap.keys, snap.flags, c->esdf_removed, g, e.use_region != 0, region_lo, region_hi, &L);
  const size_t nx = L.X.size(), ny = L.Y.size(), nz = L.Z.size();
  const uint64_t workspace = (uint64_t)(nx + ny) * kEsdfBrickKeys * 8 + (uint64_t)(nx + ny + nz) * 8 + (uint64_t)nz * 4;
  if (stats) {
    stats->tiles_stale = L.n_stale;
    stats->tiles_recomputed = nz;
    stats->tiles_total = nt;
    stats->voxels_observed = c->esdf_totals[0];
    stats->voxels_fixed = c->esdf_totals[1];
    stats->voxels_clamped = c->esdf_totals[2];
    stats->workspace_bytes = (L.n_stale || tiles_left) ? workspace : 0;
  }
  if (L.n_stale == 0 && !tiles_left) {   // nothing to do: the totals of the store as it is
    c->esdf_changed.clear();
    c->nav_valid = false;   // the navigation field does not outlive a successful refresh, whatever it recomputed
    drop_frontiers(c);      // ... nor do the frontiers (§21)
    drop_rooms(c);          // ... nor the rooms (§25)
    return KS_OK;
  }
  if (workspace > max_workspace_bytes) {
    c->err = "ks_esdf_refresh: " + std::to_string(nz) + " tiles to recompute need " + std::to_string(workspace) +
             " bytes of work space, more than max_workspace_bytes = " + std::to_string(max_workspace_bytes);
    return KS_ERR_UNSUPPORTED;
  }
  if (nx >= (1ull << 31) || ny >= (1ull << 31)) {
    c->err = "ks_esdf_refresh: too many tiles for one call";
    return KS_ERR_UNSUPPORTED;
  }
  // 2) room for the tiles that joined: the store keeps its records when it moves
  DevBuf<EsdfRecord> grown;
  if ((size_t)nt * kTileVoxels > c->esdf_store.size())
    if ((rc = grown.alloc(c, ((size_t)nt + nt / 2 + 64) * kTileVoxels))) return rc;
  if ((rc = c->esdf_bricks[0].reserve(c, nx * kEsdfBrickKeys, (nx + nx / 2) * kEsdfBrickKeys)) ||
      (rc = c->esdf_bricks[1].reserve(c, ny * kEsdfBrickKeys, (ny + ny / 2) * kEsdfBrickKeys)) ||
      (rc = c->esdf_lists.reserve(c, nx + ny + nz, (nx + ny + nz) * 3 / 2)) || (rc = c->esdf_zslots.reserve(c, nz, nz * 3 / 2)) ||
      (rc = c->esdf_counters.reserve(c, 3, 3)))
    return rc;
  c->esdf_valid = false;   // (a failure below leaves no half-written store readable)
  c->nav_valid = false;    // the navigation field is a snapshot of the store as it was
  drop_frontiers(c);       // ... and so are the frontiers (§21)
  drop_rooms(c);           // ... and the rooms (§25)
  if (grown.get()) {
    if (nt_old) HIPCHK(c, hipMemcpyAsync(grown.get(), c->esdf_store.get(), (size_t)nt_old * kTileVoxels * sizeof(EsdfRecord), hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    c->esdf_store = std::move(grown);
  }
  if (nt > nt_old)
    hipLaunchKernelGGL(k_esdf_fill, dim3((uint32_t)(((size_t)(nt - nt_old) * kTileVoxels + 255) / 256)), dim3(256), 0, st,
                       c->esdf_store.get() + (size_t)nt_old * kTileVoxels, (size_t)(nt - nt_old) * kTileVoxels);
  unsigned long long counts[3] = {c->esdf_totals[0], c->esdf_totals[1], c->esdf_totals[2]};
  if (nz) {
    // 3) the three passes over the lists, then the totals from the records
    uint64_t* d_x = c->esdf_lists.get();
    uint64_t *d_y = d_x + nx, *d_z = d_y + ny;
    if (nx) HIPCHK(c, hipMemcpyAsync(d_x, L.X.data(), nx * 8, hipMemcpyHostToDevice, st));
    if (ny) HIPCHK(c, hipMemcpyAsync(d_y, L.Y.data(), ny * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_z, L.Z.data(), nz * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->esdf_zslots, L.z_slots.data(), nz * 4, hipMemcpyHostToDevice, st));
    EsdfRefresh E{R, c->cfg.voxel_size, e.min_weight, e.min_distance_m, e.max_distance_m};
    if (nx)
      hipLaunchKernelGGL(k_esdf_brick<0>, dim3((uint32_t)nx), dim3(256), 0, st, E, c->table, c->pool, nt, (const uint64_t*)d_x,
                         (const uint64_t*)nullptr, 0u, (const uint64_t*)nullptr, c->esdf_bricks[0].get(), (const uint32_t*)nullptr,
                         (EsdfRecord*)nullptr);
    if (ny)
      hipLaunchKernelGGL(k_esdf_brick<1>, dim3((uint32_t)ny), dim3(256), 0, st, E, c->table, c->pool, nt, (const uint64_t*)d_y,
                         (const uint64_t*)d_x, (uint32_t)nx, (const uint64_t*)c->esdf_bricks[0].get(), c->esdf_bricks[1].get(),
                         (const uint32_t*)nullptr, (EsdfRecord*)nullptr);
    hipLaunchKernelGGL(k_esdf_brick<2>, dim3((uint32_t)nz), dim3(256), 0, st, E, c->table, c->pool, nt, (const uint64_t*)d_z,
                       (const uint64_t*)d_y, (uint32_t)ny, (const uint64_t*)c->esdf_bricks[1].get(), (uint64_t*)nullptr,
                       (const uint32_t*)c->esdf_zslots.get(), c->esdf_store.get());
  }
  if (nt) {   // (after a removal also with nothing to recompute: the records of the tiles that left no longer count)
    const size_t nrec = (size_t)nt * kTileVoxels;
    HIPCHK(c, hipMemsetAsync(c->esdf_counters, 0, 3 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_esdf_count, dim3((uint32_t)((nrec + 1023) / 1024)), dim3(256), 0, st, (const EsdfRecord*)c->esdf_store.get(), nrec,
                       e.max_distance_m, c->esdf_counters.get());
    HIPCHK(c, hipMemcpyAsync(counts, c->esdf_counters, sizeof(counts), hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(k_stale_clear, dim3((nt + 255) / 256), dim3(256), 0, st, c->pool.mesh_stale(), nt, kStaleEsdf);
  } else {
    counts[0] = counts[1] = counts[2] = 0;   // (every tile has left)
  }
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  c->esdf_valid = true;
  c->esdf_tiles = nt;
  c->esdf_removed.clear();
  for (int k = 0; k < 3; ++k) c->esdf_totals[k] = counts[k];
  // 4) the blocks of the recomputed tiles
  words_to_triples(blocks_of_tiles(L.Z, c->vps_shift), &c->esdf_changed);
  if (stats) {
    stats->voxels_observed = counts[0];
    stats->voxels_fixed = counts[1];
    stats->voxels_clamped = counts[2];
  }
  return KS_OK;
}

int ks_esdf_changed_blocks(ks_ctx* c, int32_t* out_xyz, size_t cap, size_t* n) {
  return c ? copy_block_list(c, "ks_esdf_changed_blocks", c->esdf_changed, out_xyz, cap, n) : KS_ERR_INVALID_ARG;
}

int ks_esdf_download_blocks(ks_ctx* c, const int32_t* idx, size_t n, void* out) {
  if (!c || (n && (!idx || !out))) return KS_ERR_INVALID_ARG;
  if (int rc = esdf_ready(c, "ks_esdf_download_blocks")) return rc;
  if (n == 0) return KS_OK;
  if (int rc = quiesce(c)) return rc;
  const int vps = c->cfg.voxels_per_side;
  const size_t nv = (size_t)vps * vps * vps;
  const size_t chunk = std::min<size_t>(std::max<size_t>(1, (size_t(64) << 20) / (nv * sizeof(EsdfRecord))), 65535);   // <= 64 MiB staged at a time
  const size_t m_max = std::min(chunk, n);
  int rc;
  if ((rc = c->esdf_out.reserve(c, m_max * nv, m_max * nv))) return rc;
  if ((rc = c->esdf_idx.reserve(c, m_max * 3, m_max * 3))) return rc;
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->esdf_idx, idx + 3 * off, m * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_esdf_download, dim3((uint32_t)((nv + 255) / 256), (uint32_t)m), dim3(256), 0, c->stream, c->table,
                       (const EsdfRecord*)c->esdf_store.get(), c->esdf_tiles, (const int32_t*)c->esdf_idx.get(), vps, c->esdf_out.get());
    HIPCHK(c, hipMemcpyAsync((uint8_t*)out + off * nv * sizeof(EsdfRecord), c->esdf_out, m * nv * sizeof(EsdfRecord), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

int ks_esdf_query(ks_ctx* c, const float* xyz, size_t n, float* distance, uint8_t* flags, uint8_t* label) {
  if (!c || (n && !xyz)) return KS_ERR_INVALID_ARG;
  if (int rc = esdf_ready(c, "ks_esdf_query")) return rc;
  if (n == 0) return KS_OK;
  if (int rc = quiesce(c)) return rc;
  const size_t chunk = size_t(1) << 22;
  const size_t m_max = std::min(chunk, n);
  int rc;
  if ((rc = c->esdf_out.reserve(c, m_max, m_max))) return rc;
  if ((rc = c->esdf_xyz.reserve(c, m_max * 3, m_max * 3))) return rc;
  std::vector<EsdfRecord> rec(m_max);
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->esdf_xyz, xyz + 3 * off, m * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_esdf_query, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, c->stream, c->table, (const EsdfRecord*)c->esdf_store.get(),
                       c->esdf_tiles, (const float*)c->esdf_xyz.get(), m, c->voxel_size_inv, c->esdf_out.get());
    HIPCHK(c, hipMemcpyAsync(rec.data(), c->esdf_out, m * sizeof(EsdfRecord), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < m; ++i) {
      if (distance) distance[off + i] = rec[i].distance;
      if (flags) flags[off + i] = (uint8_t)(rec[i].tail & 0xffu);
      if (label) label[off + i] = (uint8_t)((rec[i].tail >> 8) & 0xffu);
    }
  }
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

// ---- reads of the stored ESDF ("ESDF reads"; ks_k_esdf_read.h) ----------------------------------
// what all six calls ask of the context, then the frames in flight are completed
static int esdf_read_begin(ks_ctx* c, const char* who) {
  if (int rc = holds_voxels(c, who)) return rc;
  if (c->fatal) {
    c->err = std::string(who) + ": context is in a failed state (earlier pool/index error)";
    return KS_ERR_INVALID_ARG;
  }
  if (int rc = esdf_ready(c, who)) return rc;
  if (int rc = quiesce(c)) return rc;
  if (int rc = c->esdf_read_counters.reserve(c, 8, 8)) return rc;
  HIPCHK(c, hipMemsetAsync(c->esdf_read_counters, 0, 8 * sizeof(unsigned long long), c->stream));
  return KS_OK;
}
static int esdf_read_refuse(ks_ctx* c, const char* who, const char* why) {
  c->err = std::string(who) + ": " + why;
  return KS_ERR_INVALID_ARG;
}
static EsdfReadStore esdf_read_view(ks_ctx* c) { return EsdfReadStore{c->esdf_store.get(), c->esdf_tiles, c->voxel_size_inv}; }
// waits for the stream and reads k counters
static int esdf_read_counts(ks_ctx* c, uint64_t* out, int k) {
  unsigned long long counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(counts, c->esdf_read_counters, (size_t)k * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int a = 0; a < k; ++a) out[a] = counts[a];
  return KS_OK;
}
static int esdf_sample_stats(ks_ctx* c, ks_esdf_sample_stats* stats) {
  uint64_t v[3];
  if (int rc = esdf_read_counts(c, v, 3)) return rc;
  stats->points_interpolated = v[0];
  stats->points_nearest = v[1];
  stats->points_unknown = v[2];
  return KS_OK;
}
// the five staged outputs of m points (or pixels) to the caller's arrays at element `off`; O holds the staging addresses
static int esdf_sample_copy_out(ks_ctx* c, const EsdfSampleOut& O, size_t off, size_t m, float* distance, float* gradient, uint8_t* status,
                                uint8_t* label, uint8_t* flags) {
  hipStream_t st = c->stream;
  if (distance) HIPCHK(c, hipMemcpyAsync(distance + off, O.distance, m * sizeof(float), hipMemcpyDeviceToHost, st));
  if (gradient) HIPCHK(c, hipMemcpyAsync(gradient + 3 * off, O.gradient, 3 * m * sizeof(float), hipMemcpyDeviceToHost, st));
  if (status) HIPCHK(c, hipMemcpyAsync(status + off, O.status, m, hipMemcpyDeviceToHost, st));
  if (label) HIPCHK(c, hipMemcpyAsync(label + off, O.label, m, hipMemcpyDeviceToHost, st));
  if (flags) HIPCHK(c, hipMemcpyAsync(flags + off, O.flags, m, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));   // (the staging is reused by the next chunk)
  return KS_OK;
}
// room for m_max points (or pixels) in the staging of the host-pointer calls, and where each wanted output lies in it
static int esdf_sample_staging(ks_ctx* c, size_t m_max, bool distance, bool gradient, bool status, bool label, bool flags, EsdfSampleOut* O) {
  int rc;
  if ((rc = c->esdf_read_f.reserve(c, 4 * m_max, 4 * m_max)) || (rc = c->esdf_read_b.reserve(c, 3 * m_max, 3 * m_max))) return rc;
  O->distance = distance ? c->esdf_read_f.get() : nullptr;
  O->gradient = gradient ? c->esdf_read_f.get() + m_max : nullptr;
  O->status = status ? c->esdf_read_b.get() : nullptr;
  O->label = label ? c->esdf_read_b.get() + m_max : nullptr;
  O->flags = flags ? c->esdf_read_b.get() + 2 * m_max : nullptr;
  O->counters = c->esdf_read_counters;
  return KS_OK;
}
// k_esdf_sample over n points at a DEVICE address (a launch takes at most 2^30 of them)
static void esdf_sample_launch(ks_ctx* c, const float* d_xyz, size_t n, const EsdfSampleOut& O) {
  const size_t per = size_t(1) << 30;
  for (size_t off = 0; off < n; off += per) {
    const size_t m = std::min(per, n - off);
    EsdfSampleOut P = O;
    if (P.distance) P.distance += off;
    if (P.gradient) P.gradient += 3 * off;
    if (P.status) P.status += off;
    if (P.label) P.label += off;
    if (P.flags) P.flags += off;
    hipLaunchKernelGGL(k_esdf_sample, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, c->stream, c->table, esdf_read_view(c), d_xyz + 3 * off, m, P);
  }
}

int ks_esdf_sample_device(ks_ctx* c, const float* d_xyz, size_t n, float* d_distance, float* d_gradient, uint8_t* d_status, uint8_t* d_label,
                          uint8_t* d_flags, ks_esdf_sample_stats* stats) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const char* who = "ks_esdf_sample_device";
  if (n && !d_xyz) return esdf_read_refuse(c, who, "xyz is NULL");
  if (n && !d_distance && !d_gradient && !d_status && !d_label && !d_flags) return esdf_read_refuse(c, who, "all five outputs are NULL");
  if (int rc = esdf_read_begin(c, who)) return rc;
  if (n == 0) return KS_OK;
  esdf_sample_launch(c, d_xyz, n, EsdfSampleOut{d_distance, d_gradient, d_status, d_label, d_flags, c->esdf_read_counters});
  HIPCHK(c, hipGetLastError());
  return stats ? esdf_sample_stats(c, stats) : KS_OK;
}

int ks_esdf_sample(ks_ctx* c, const float* xyz, size_t n, float* distance, float* gradient, uint8_t* status, uint8_t* label, uint8_t* flags,
                   ks_esdf_sample_stats* stats) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const char* who = "ks_esdf_sample";
  if (n && !xyz) return esdf_read_refuse(c, who, "xyz is NULL");
  if (n && !distance && !gradient && !status && !label && !flags) return esdf_read_refuse(c, who, "all five outputs are NULL");
  if (int rc = esdf_read_begin(c, who)) return rc;
  if (n == 0) return KS_OK;
  const size_t m_max = std::min(c->esdf_read_chunk, n);
  EsdfSampleOut O{};
  int rc;
  if ((rc = c->esdf_read_in.reserve(c, 3 * m_max, 3 * m_max)) || (rc = esdf_sample_staging(c, m_max, distance, gradient, status, label, flags, &O))) return rc;
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->esdf_read_in, xyz + 3 * off, 3 * m * sizeof(float), hipMemcpyHostToDevice, c->stream));
    esdf_sample_launch(c, c->esdf_read_in, m, O);
    if ((rc = esdf_sample_copy_out(c, O, off, m, distance, gradient, status, label, flags))) return rc;
  }
  HIPCHK(c, hipGetLastError());
  return stats ? esdf_sample_stats(c, stats) : KS_OK;
}

// the checks of both slice calls
static int esdf_slice_check(ks_ctx* c, const char* who, const float origin[3], const float du[3], const float dv[3], int width, int height,
                            bool any_output) {
  if (!origin || !du || !dv) return esdf_read_refuse(c, who, "origin, du or dv is NULL");
  if (width < 1 || width > 8192 || height < 1 || height > 8192) return esdf_read_refuse(c, who, "width and height must lie in 1..8192");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(origin[k]) || !std::isfinite(du[k]) || !std::isfinite(dv[k])) return esdf_read_refuse(c, who, "origin, du and dv must be finite");
  if (!any_output) return esdf_read_refuse(c, who, "all five outputs are NULL");
  return KS_OK;
}
static void esdf_slice_launch(ks_ctx* c, const float origin[3], const float du[3], const float dv[3], int width, int row0, int rows,
                              const EsdfSampleOut& O) {
  EsdfSlice V{};
  for (int k = 0; k < 3; ++k) {
    V.origin[k] = origin[k];
    V.du[k] = du[k];
    V.dv[k] = dv[k];
  }
  V.width = width;
  V.row0 = row0;
  V.rows = rows;
  hipLaunchKernelGGL(k_esdf_slice, dim3((uint32_t)((width + 15) / 16), (uint32_t)((rows + 15) / 16)), dim3(256), 0, c->stream, c->table,
                     esdf_read_view(c), V, O);
}

int ks_esdf_slice_device(ks_ctx* c, const float origin[3], const float du[3], const float dv[3], int width, int height, float* d_distance,
                         float* d_gradient, uint8_t* d_status, uint8_t* d_label, uint8_t* d_flags, ks_esdf_sample_stats* stats) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const char* who = "ks_esdf_slice_device";
  if (int rc = esdf_slice_check(c, who, origin, du, dv, width, height, d_distance || d_gradient || d_status || d_label || d_flags)) return rc;
  if (int rc = esdf_read_begin(c, who)) return rc;
  esdf_slice_launch(c, origin, du, dv, width, 0, height, EsdfSampleOut{d_distance, d_gradient, d_status, d_label, d_flags, c->esdf_read_counters});
  HIPCHK(c, hipGetLastError());
  return stats ? esdf_sample_stats(c, stats) : KS_OK;
}

int ks_esdf_slice(ks_ctx* c, const float origin[3], const float du[3], const float dv[3], int width, int height, float* distance, float* gradient,
                  uint8_t* status, uint8_t* label, uint8_t* flags, ks_esdf_sample_stats* stats) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const char* who = "ks_esdf_slice";
  if (int rc = esdf_slice_check(c, who, origin, du, dv, width, height, distance || gradient || status || label || flags)) return rc;
  if (int rc = esdf_read_begin(c, who)) return rc;
  // bands of whole rows, about a chunk of pixels each
  const int band = (int)std::min<size_t>((size_t)height, std::max<size_t>(1, c->esdf_read_chunk / (size_t)width));
  const size_t m_max = (size_t)band * (size_t)width;
  EsdfSampleOut O{};
  int rc;
  if ((rc = esdf_sample_staging(c, m_max, distance, gradient, status, label, flags, &O))) return rc;
  for (int row0 = 0; row0 < height; row0 += band) {
    const int rows = std::min(band, height - row0);
    esdf_slice_launch(c, origin, du, dv, width, row0, rows, O);
    if ((rc = esdf_sample_copy_out(c, O, (size_t)row0 * (size_t)width, (size_t)rows * (size_t)width, distance, gradient, status, label, flags))) return rc;
  }
  HIPCHK(c, hipGetLastError());
  return stats ? esdf_sample_stats(c, stats) : KS_OK;
}

int ks_esdf_sweep_default_config(ks_esdf_sweep_config* s) {
  if (!s) return KS_ERR_INVALID_ARG;
  s->radius_m = 0.3f;
  s->min_step_m = 0.0f;
  s->unknown_is_free = 0;
  s->max_samples = 4096;
  return KS_OK;
}

// the checks of both sweep calls and the kernel's parameters but for its pointers
static int esdf_sweep_check(ks_ctx* c, const char* who, size_t n, const ks_esdf_sweep_config* s, EsdfSweep* W) {
  if (!s) return esdf_read_refuse(c, who, "the configuration is NULL");
  if (!std::isfinite(s->radius_m) || s->radius_m < 0.0f || !std::isfinite(s->min_step_m) || s->min_step_m < 0.0f)
    return esdf_read_refuse(c, who, "radius_m and min_step_m must be finite and not negative");
  if (s->max_samples < 2 || s->max_samples > 65536) return esdf_read_refuse(c, who, "max_samples must lie in 2..65536");
  if ((uint64_t)n >= (1ull << 32)) return esdf_read_refuse(c, who, "2^32 segments or more in one call");
  W->radius = s->radius_m;
  W->min_step = s->min_step_m > 0.0f ? s->min_step_m : 0.5f * c->cfg.voxel_size;
  W->max_length = (float)(s->max_samples - 2) * W->min_step;
  W->unknown_is_free = s->unknown_is_free != 0;
  W->max_samples = s->max_samples;
  return KS_OK;
}
static int esdf_sweep_stats(ks_ctx* c, ks_esdf_sweep_stats* stats) {
  uint64_t v[5];
  if (int rc = esdf_read_counts(c, v, 5)) return rc;
  stats->segments_free = v[0];
  stats->segments_collision = v[1];
  stats->segments_unknown = v[2];
  stats->segments_invalid = v[3];
  stats->samples = v[4];
  return KS_OK;
}
// k_esdf_sweep over W.n segments at a DEVICE address (a launch takes at most 2^30 of them)
static void esdf_sweep_launch(ks_ctx* c, const EsdfSweep& W) {
  const size_t per = size_t(1) << 30;
  for (size_t off = 0; off < W.n; off += per) {
    EsdfSweep P = W;
    P.n = std::min(per, W.n - off);
    P.segments += 6 * off;
    if (P.status) P.status += off;
    if (P.t_stop) P.t_stop += off;
    if (P.min_clearance) P.min_clearance += off;
    if (P.t_min) P.t_min += off;
    hipLaunchKernelGGL(k_esdf_sweep, dim3((uint32_t)((P.n + 255) / 256)), dim3(256), 0, c->stream, c->table, esdf_read_view(c), P);
  }
}

int ks_esdf_sweep_device(ks_ctx* c, const float* d_segments, size_t n, const ks_esdf_sweep_config* s, uint8_t* d_status, float* d_t_stop,
                         float* d_min_clearance, float* d_t_min, ks_esdf_sweep_stats* stats) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const char* who = "ks_esdf_sweep_device";
  EsdfSweep W{};
  if (int rc = esdf_sweep_check(c, who, n, s, &W)) return rc;
  if (n && !d_segments) return esdf_read_refuse(c, who, "segments is NULL");
  if (n && !d_status && !d_t_stop && !d_min_clearance && !d_t_min) return esdf_read_refuse(c, who, "all four outputs are NULL");
  if (int rc = esdf_read_begin(c, who)) return rc;
  if (n == 0) return KS_OK;
  W.segments = d_segments;
  W.n = n;
  W.status = d_status;
  W.t_stop = d_t_stop;
  W.min_clearance = d_min_clearance;
  W.t_min = d_t_min;
  W.counters = c->esdf_read_counters;
  esdf_sweep_launch(c, W);
  HIPCHK(c, hipGetLastError());
  return stats ? esdf_sweep_stats(c, stats) : KS_OK;
}

int ks_esdf_sweep(ks_ctx* c, const float* segments, size_t n, const ks_esdf_sweep_config* s, uint8_t* status, float* t_stop, float* min_clearance,
                  float* t_min, ks_esdf_sweep_stats* stats) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const char* who = "ks_esdf_sweep";
  EsdfSweep W{};
  if (int rc = esdf_sweep_check(c, who, n, s, &W)) return rc;
  if (n && !segments) return esdf_read_refuse(c, who, "segments is NULL");
  if (n && !status && !t_stop && !min_clearance && !t_min) return esdf_read_refuse(c, who, "all four outputs are NULL");
  if (int rc = esdf_read_begin(c, who)) return rc;
  if (n == 0) return KS_OK;
  const size_t m_max = std::min(c->esdf_read_chunk, n);
  int rc;
  if ((rc = c->esdf_read_in.reserve(c, 6 * m_max, 6 * m_max)) || (rc = c->esdf_read_f.reserve(c, 3 * m_max, 3 * m_max)) ||
      (rc = c->esdf_read_b.reserve(c, m_max, m_max)))
    return rc;
  W.segments = c->esdf_read_in;
  W.status = status ? c->esdf_read_b.get() : nullptr;
  W.t_stop = t_stop ? c->esdf_read_f.get() : nullptr;
  W.min_clearance = min_clearance ? c->esdf_read_f.get() + m_max : nullptr;
  W.t_min = t_min ? c->esdf_read_f.get() + 2 * m_max : nullptr;
  W.counters = c->esdf_read_counters;
  hipStream_t st = c->stream;
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->esdf_read_in, segments + 6 * off, 6 * m * sizeof(float), hipMemcpyHostToDevice, st));
    W.n = m;
    esdf_sweep_launch(c, W);
    if (status) HIPCHK(c, hipMemcpyAsync(status + off, W.status, m, hipMemcpyDeviceToHost, st));
    if (t_stop) HIPCHK(c, hipMemcpyAsync(t_stop + off, W.t_stop, m * sizeof(float), hipMemcpyDeviceToHost, st));
    if (min_clearance) HIPCHK(c, hipMemcpyAsync(min_clearance + off, W.min_clearance, m * sizeof(float), hipMemcpyDeviceToHost, st));
    if (t_min) HIPCHK(c, hipMemcpyAsync(t_min + off, W.t_min, m * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));   // (the staging is reused by the next chunk)
  }
  HIPCHK(c, hipGetLastError());
  return stats ? esdf_sweep_stats(c, stats) : KS_OK;
}

// ---- view rendering ("View rendering"; ks_k_render.h) -------------------------------------------
int ks_render_default_config(ks_render_config* r) {
  if (!r) return KS_ERR_INVALID_ARG;
  r->min_weight = 1e-4f;
  r->min_range_m = 0.1f;
  r->max_range_m = 10.0f;
  return KS_OK;
}

// the checks of both calls, then the kernel on the context's stream into DEVICE images; the host is not waited for here
static int render_enqueue(ks_ctx* c, const char* who, const float T[7], const float K[4], int width, int height, const ks_render_config* r,
                          float* d_depth, uint8_t* d_labels, uint8_t* d_rgba, float* d_normals) {
  auto refuse = [&](const char* why) {
    c->err = std::string(who) + ": " + why;
    return KS_ERR_INVALID_ARG;
  };
  if (width < 1 || width > 8192 || height < 1 || height > 8192) return refuse("width and height must lie in 1..8192");
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(K[k])) return refuse("K must be finite");
  if (!(K[0] > 0.0f) || !(K[1] > 0.0f)) return refuse("fx and fy must be positive");
  const float par[3] = {r->min_weight, r->min_range_m, r->max_range_m};
  for (float v : par)
    if (!std::isfinite(v) || !(v > 0.0f)) return refuse("min_weight, min_range_m and max_range_m must be finite positive numbers");
  if (r->min_range_m >= r->max_range_m) return refuse("min_range_m must be below max_range_m");
  if (r->max_range_m / c->cfg.voxel_size > 4096.0f) return refuse("max_range_m is more than 4096 voxels");
  if (!d_depth && !d_labels && !d_rgba && !d_normals) return refuse("all four outputs are NULL");
  if (int rc = holds_voxels(c, who)) return rc;
  if (int rc = quiesce(c)) return rc;
  if (int rc = c->render_counters.reserve(c, 3, 3)) return rc;
  RenderView V{};
  V.T.w = T[0];
  V.T.v = {T[1], T[2], T[3]};
  V.T.t = {T[4], T[5], T[6]};
  V.cx = K[2];
  V.cy = K[3];
  V.constant_x = (float)(1.0 / (double)K[0]);   // as the f32 depth format of ks_integrate_depth
  V.constant_y = (float)(1.0 / (double)K[1]);
  V.width = width;
  V.height = height;
  V.voxel_size = c->cfg.voxel_size;
  V.voxel_size_inv = c->voxel_size_inv;
  V.min_weight = r->min_weight;
  V.min_range = r->min_range_m;
  V.max_range = r->max_range_m;
  V.n_tiles = c->tiles_initialised;
  V.depth = d_depth;
  V.labels = d_labels;
  V.rgba = (uint32_t*)d_rgba;
  V.normals = d_normals;
  V.counters = c->render_counters;
  HIPCHK(c, hipMemsetAsync(c->render_counters, 0, 3 * sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(k_render_view, dim3((uint32_t)((width + 15) / 16), (uint32_t)((height + 15) / 16)), dim3(256), 0, c->stream, c->table, c->pool, V);
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

// waits for the stream and reads the three counters
static int render_stats(ks_ctx* c, ks_render_stats* stats) {
  unsigned long long counts[3] = {0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(counts, c->render_counters, sizeof(counts), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  stats->pixels_hit = counts[0];
  stats->pixels_missed = counts[1];
  stats->samples = counts[2];
  return KS_OK;
}

int ks_render_view_device(ks_ctx* c, const float T[7], const float K[4], int width, int height, const ks_render_config* r, float* d_depth,
                          uint8_t* d_labels, uint8_t* d_rgba, float* d_normals, ks_render_stats* stats) {
  if (!c || !T || !K || !r) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (int rc = render_enqueue(c, "ks_render_view_device", T, K, width, height, r, d_depth, d_labels, d_rgba, d_normals)) return rc;
  return stats ? render_stats(c, stats) : KS_OK;
}

int ks_render_view(ks_ctx* c, const float T[7], const float K[4], int width, int height, const ks_render_config* r, float* depth,
                   uint8_t* labels, uint8_t* rgba, float* normals, ks_render_stats* stats) {
  if (!c || !T || !K || !r) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const size_t n = width > 0 && height > 0 && width <= 8192 && height <= 8192 ? (size_t)width * (size_t)height : 0;   // (0: refused below)
  int rc;
  if (n && depth && (rc = c->render_depth.reserve(c, n, n))) return rc;
  if (n && labels && (rc = c->render_labels.reserve(c, n, n))) return rc;
  if (n && rgba && (rc = c->render_rgba.reserve(c, n, n))) return rc;
  if (n && normals && (rc = c->render_normals.reserve(c, 3 * n, 3 * n))) return rc;
  if ((rc = render_enqueue(c, "ks_render_view", T, K, width, height, r, depth ? c->render_depth.get() : nullptr,
                           labels ? c->render_labels.get() : nullptr, rgba ? (uint8_t*)c->render_rgba.get() : nullptr,
                           normals ? c->render_normals.get() : nullptr)))
    return rc;
  hipStream_t st = c->stream;
  if (depth) HIPCHK(c, hipMemcpyAsync(depth, c->render_depth, n * sizeof(float), hipMemcpyDeviceToHost, st));
  if (labels) HIPCHK(c, hipMemcpyAsync(labels, c->render_labels, n, hipMemcpyDeviceToHost, st));
  if (rgba) HIPCHK(c, hipMemcpyAsync(rgba, c->render_rgba, n * 4, hipMemcpyDeviceToHost, st));
  if (normals) HIPCHK(c, hipMemcpyAsync(normals, c->render_normals, 3 * n * sizeof(float), hipMemcpyDeviceToHost, st));
  if (stats) return render_stats(c, stats);
  HIPCHK(c, hipStreamSynchronize(st));
  return KS_OK;
}

// ---- scan alignment ("Scan alignment"; ks_k_align.h) --------------------------------------------
int ks_align_default_config(ks_align_config* a) {
  if (!a) return KS_ERR_INVALID_ARG;
  a->min_weight = 1e-4f;
  a->max_residual_m = 0.0f;
  a->damping = 1e-6f;
  a->eps_rotation_rad = 1e-4f;
  a->eps_translation_m = 1e-4f;
  a->max_iterations = 10;
  a->point_stride = 1;
  a->min_inliers = 64;
  a->dof_mask = 0x3fu;
  return KS_OK;
}

// the checks of both calls, then the whole loop on the context's stream: max_iterations pairs (evaluate, finish) and the
// last pair, one read-back of the state block, one host wait
static int align_run(ks_ctx* c, const char* who, const float T[7], const float* d_xyz, size_t n, const ks_align_config* a, float T_out[7],
                     ks_align_stats* stats) {
  AlignParams A{};
  A.xyz = d_xyz;
  A.n = (uint32_t)n;
  A.stride = (uint32_t)a->point_stride;
  A.n_used = (uint32_t)((n + (size_t)a->point_stride - 1) / (size_t)a->point_stride);
  A.n_waves = (A.n_used + 63u) / 64u;
  A.voxel_size_inv = c->voxel_size_inv;
  A.min_weight = a->min_weight;
  A.max_residual = a->max_residual_m > 0.0f ? a->max_residual_m : c->cfg.truncation_distance;
  A.n_tiles = c->tiles_initialised;
  A.damping = a->damping;
  A.eps_rotation = a->eps_rotation_rad;
  A.eps_translation = a->eps_translation_m;
  A.max_iterations = a->max_iterations;
  A.min_inliers = a->min_inliers;
  A.dof_mask = a->dof_mask;
  const size_t n_partials = (size_t)kAlignSums * std::max<size_t>(A.n_waves, 1);
  if (int rc = c->align_partials.reserve(c, n_partials, n_partials)) return rc;
  if (int rc = c->align_state.reserve(c, 1, 1)) return rc;
  A.partials = c->align_partials;
  A.state = c->align_state;
  AlignState S{};
  for (int k = 0; k < 4; ++k) S.q[k] = T[k];
  for (int k = 0; k < 3; ++k) S.t[k] = T[4 + k];
  S.status = KS_ALIGN_ITERATION_LIMIT;
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(c->align_state, &S, sizeof(S), hipMemcpyHostToDevice, st));
  const dim3 grid(std::max<uint32_t>((A.n_used + 255u) / 256u, 1u));
  for (int it = 0; it <= a->max_iterations; ++it) {
    const int iteration = it < a->max_iterations ? it : kAlignLast;
    hipLaunchKernelGGL(k_align_eval, grid, dim3(256), 0, st, c->table, c->pool, A, iteration);
    hipLaunchKernelGGL(k_align_finish, dim3(1), dim3(256), 0, st, A, iteration);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(&S, c->align_state, sizeof(S), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  for (int k = 0; k < 4; ++k) T_out[k] = S.q[k];
  for (int k = 0; k < 3; ++k) T_out[4 + k] = S.t[k];
  if (stats) {
    stats->status = S.status;
    stats->iterations = S.iterations;
    stats->points_used = (uint64_t)S.used;
    stats->inliers_first = (uint64_t)S.inliers_first;
    stats->inliers_last = (uint64_t)S.inliers_last;
    stats->rmse_first = S.inliers_first > 0.0 ? std::sqrt(S.rr_first / S.inliers_first) : 0.0;
    stats->rmse_last = S.inliers_last > 0.0 ? std::sqrt(S.rr_last / S.inliers_last) : 0.0;
  }
  return KS_OK;
}

static int align_check(ks_ctx* c, const char* who, const float T[7], size_t n, const ks_align_config* a) {
  auto refuse = [&](const char* why) {
    c->err = std::string(who) + ": " + why;
    return KS_ERR_INVALID_ARG;
  };
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(T[k])) return refuse("the pose must be finite");
  if (T[0] == 0.0f && T[1] == 0.0f && T[2] == 0.0f && T[3] == 0.0f) return refuse("the quaternion is zero");
  if (!std::isfinite(a->min_weight) || !(a->min_weight > 0.0f)) return refuse("min_weight must be a finite positive number");
  const float par[4] = {a->max_residual_m, a->damping, a->eps_rotation_rad, a->eps_translation_m};
  for (float v : par)
    if (!std::isfinite(v) || v < 0.0f) return refuse("max_residual_m, damping, eps_rotation_rad and eps_translation_m must be finite and not negative");
  if (a->max_iterations < 1 || a->max_iterations > 64) return refuse("max_iterations must lie in 1..64");
  if (a->point_stride < 1) return refuse("point_stride must be at least 1");
  if (a->min_inliers < 1) return refuse("min_inliers must be at least 1");
  if (a->dof_mask == 0u || a->dof_mask > 0x3fu) return refuse("dof_mask must lie in 1..0x3f");
  if (n >= ((size_t)1 << 31)) return refuse("more than 2^31 - 1 points");
  if (int rc = holds_voxels(c, who)) return rc;
  return quiesce(c);
}

int ks_align_points_device(ks_ctx* c, const float T[7], const float* d_xyz, size_t n, const ks_align_config* a, float T_out[7], ks_align_stats* stats) {
  if (!c || !T || !a || !T_out || (n && !d_xyz)) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (int rc = align_check(c, "ks_align_points_device", T, n, a)) return rc;
  return align_run(c, "ks_align_points_device", T, d_xyz, n, a, T_out, stats);
}

int ks_align_points(ks_ctx* c, const float T[7], const float* xyz, size_t n, const ks_align_config* a, float T_out[7], ks_align_stats* stats) {
  if (!c || !T || !a || !T_out || (n && !xyz)) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (int rc = align_check(c, "ks_align_points", T, n, a)) return rc;
  if (int rc = c->align_xyz.reserve(c, 3 * n, 3 * n)) return rc;
  if (n) HIPCHK(c, hipMemcpyAsync(c->align_xyz, xyz, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  return align_run(c, "ks_align_points", T, c->align_xyz, n, a, T_out, stats);
}

// ---- object instances ("Object instances"; ks_k_objects.h) --------------------------------------
int ks_objects_default_config(ks_objects_config* o) {
  if (!o) return KS_ERR_INVALID_ARG;
  o->min_weight = 1e-4f;
  o->surface_distance_m = 0.0f;
  o->label_mask = 0x1fffffu;
  o->min_voxels = 8;
  return KS_OK;
}

int ks_objects_update(ks_ctx* c, const ks_objects_config* o, ks_objects_stats* stats) {
  if (!c || !o) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  auto refuse = [&](const char* why) {
    c->err = std::string("ks_objects_update: ") + why;
    return KS_ERR_INVALID_ARG;
  };
  if (!(o->min_weight > 0.0f) || !std::isfinite(o->min_weight)) return refuse("min_weight must be a finite positive number");
  if (!(o->surface_distance_m >= 0.0f) || !std::isfinite(o->surface_distance_m)) return refuse("surface_distance_m must be finite and not negative");
  if (o->label_mask == 0 || (o->label_mask >> kObjLabels) != 0) return refuse("label_mask must name at least one of the labels 0..20 and nothing else");
  if (o->min_voxels < 1) return refuse("min_voxels must be at least 1");
  if (int rc = holds_voxels(c, "ks_objects_update")) return rc;
  if (int rc = quiesce(c)) return rc;
  hipStream_t st = c->stream;
  const uint32_t nt = c->tiles_initialised;
  if (nt >= (1u << 23)) {   // (a voxel's id is slot * 512 + local in 32 bits, all-ones = none)
    c->err = "ks_objects_update: too many tiles for one call";
    return KS_ERR_UNSUPPORTED;
  }
  const size_t nvox = (size_t)nt * kTileVoxels;
  int rc;
  c->obj_valid = false;   // (a failure below leaves nothing half-written readable)
  c->obj_count = 0;
  if ((rc = c->obj_ids.reserve(c, nvox, ((size_t)nt + nt / 2 + 64) * kTileVoxels)) || (rc = c->obj_parent.reserve(c, nvox, nvox + nvox / 2)) ||
      (rc = c->obj_cls.reserve(c, nvox, nvox + nvox / 2)) || (rc = c->obj_counters.reserve(c, 1, 1)))
    return rc;
  HIPCHK(c, hipMemsetAsync(c->obj_counters, 0, sizeof(ObjCounters), st));
  ObjParams O{};
  O.min_weight = o->min_weight;
  O.surface_distance = o->surface_distance_m == 0.0f ? c->cfg.voxel_size : o->surface_distance_m;
  O.label_mask = o->label_mask;
  O.min_voxels = o->min_voxels;
  O.nt = nt;
  ObjCounters counts{};
  uint64_t workspace = (uint64_t)nvox * 9 + sizeof(ObjCounters);   // the forest, the id store, the class bytes
  if (nt) {
    // 1) - 3) in-tile labelling, seams, flat forest and provisional numbers
    hipLaunchKernelGGL(k_obj_label, dim3(nt), dim3(512), 0, st, c->pool, O, c->obj_cls.get(), c->obj_parent.get(), c->obj_counters.get());
    hipLaunchKernelGGL(k_obj_seams, dim3(nt), dim3(512), 0, st, c->table, O, (const uint8_t*)c->obj_cls.get(), c->obj_parent.get());
    hipLaunchKernelGGL(k_obj_number, dim3(nt * 2), dim3(256), 0, st, c->obj_parent.get(), c->obj_ids.get(), c->obj_counters.get());
    HIPCHK(c, hipMemcpyAsync(&counts, c->obj_counters, sizeof(counts), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));   // the one read that sizes what follows
    const uint32_t nc = counts.n_components;
    if (nc) {
      // 4) + 5) reduce, filter, order, assign
      const size_t cap = (size_t)nc + nc / 2;
      if ((rc = c->obj_acc.reserve(c, nc, cap)) || (rc = c->obj_final.reserve(c, nc, cap)) || (rc = c->obj_records.reserve(c, nc, cap))) return rc;
      for (int k = 0; k < 2; ++k)
        if ((rc = c->obj_keys[k].reserve(c, nc, cap)) || (rc = c->obj_vals[k].reserve(c, nc, cap))) return rc;
      const dim3 per_comp((nc + 255) / 256);
      hipLaunchKernelGGL(k_obj_acc_init, per_comp, dim3(256), 0, st, c->obj_acc.get(), nc);
      hipLaunchKernelGGL(k_obj_reduce, dim3(nt * 2), dim3(256), 0, st, c->table, (const uint8_t*)c->obj_cls.get(), c->obj_parent.get(),
                         (const uint32_t*)c->obj_ids.get(), c->obj_acc.get());
      hipLaunchKernelGGL(k_obj_keys, per_comp, dim3(256), 0, st, (const ObjAcc*)c->obj_acc.get(), nc, O.min_voxels, c->obj_keys[0].get(),
                         c->obj_vals[0].get(), c->obj_counters.get());
      uint64_t* keys = nullptr;
      uint32_t* vals = nullptr;
      if ((rc = sort_pairs(c, c->obj_keys[0].get(), c->obj_keys[1].get(), c->obj_vals[0].get(), c->obj_vals[1].get(), nc, 64, &keys, &vals))) return rc;
      hipLaunchKernelGGL(k_obj_records, per_comp, dim3(256), 0, st, (const ObjAcc*)c->obj_acc.get(), nc, (const uint64_t*)keys, (const uint32_t*)vals,
                         c->obj_records.get(), c->obj_final.get());
      workspace += (uint64_t)nc * (sizeof(ObjAcc) + sizeof(ks_object) + 2 * 8 + 3 * 4);
    }
    hipLaunchKernelGGL(k_obj_ids, dim3((uint32_t)((nvox + 255) / 256)), dim3(256), 0, st, (const uint32_t*)c->obj_parent.get(),
                       (const uint32_t*)c->obj_final.get(), c->obj_ids.get(), nvox);
    HIPCHK(c, hipMemcpyAsync(&counts, c->obj_counters, sizeof(counts), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  c->obj_valid = true;
  c->obj_tiles = nt;
  c->obj_count = counts.n_objects;
  if (stats) {
    stats->voxels_surface = counts.voxels_surface;
    stats->components = counts.n_components;
    stats->objects = counts.n_objects;
    stats->voxels_in_objects = counts.voxels_in_objects;
    stats->largest_object_voxels = counts.largest;
    stats->workspace_bytes = workspace;
  }
  return KS_OK;
}

static int objects_ready(ks_ctx* c, const char* who) {
  if (c->obj_valid) return KS_OK;
  c->err = std::string(who) + ": no objects are stored (ks_objects_update has not run since the map was created or cleared)";
  return KS_ERR_INVALID_ARG;
}

int ks_objects_size(ks_ctx* c, size_t* n) {
  if (!c || !n) return KS_ERR_INVALID_ARG;
  if (int rc = objects_ready(c, "ks_objects_size")) return rc;
  *n = c->obj_count;
  return KS_OK;
}

int ks_objects_download(ks_ctx* c, ks_object* out, size_t cap, size_t* n) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (int rc = objects_ready(c, "ks_objects_download")) return rc;
  if (n) *n = c->obj_count;
  if (cap < c->obj_count || (c->obj_count && !out)) {
    c->err = "ks_objects_download: output buffer too small";
    return KS_ERR_INVALID_ARG;
  }
  if (c->obj_count) HIPCHK(c, hipMemcpy(out, c->obj_records.get(), c->obj_count * sizeof(ks_object), hipMemcpyDeviceToHost));
  return KS_OK;
}

int ks_objects_download_blocks(ks_ctx* c, const int32_t* idx, size_t n, uint32_t* out) {
  if (!c || (n && (!idx || !out))) return KS_ERR_INVALID_ARG;
  if (int rc = objects_ready(c, "ks_objects_download_blocks")) return rc;
  if (n == 0) return KS_OK;
  if (int rc = quiesce(c)) return rc;
  const int vps = c->cfg.voxels_per_side;
  const size_t nv = (size_t)vps * vps * vps;
  const size_t chunk = std::min<size_t>(std::max<size_t>(1, (size_t(64) << 20) / (nv * sizeof(uint32_t))), 65535);   // <= 64 MiB staged at a time
  const size_t m_max = std::min(chunk, n);
  int rc;
  if ((rc = c->obj_out.reserve(c, m_max * nv, m_max * nv))) return rc;
  if ((rc = c->obj_idx.reserve(c, m_max * 3, m_max * 3))) return rc;
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->obj_idx, idx + 3 * off, m * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_obj_download, dim3((uint32_t)((nv + 255) / 256), (uint32_t)m), dim3(256), 0, c->stream, c->table,
                       (const uint32_t*)c->obj_ids.get(), c->obj_tiles, (const int32_t*)c->obj_idx.get(), vps, c->obj_out.get());
    HIPCHK(c, hipMemcpyAsync(out + off * nv, c->obj_out, m * nv * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

int ks_objects_query(ks_ctx* c, const float* xyz, size_t n, uint32_t* id) {
  if (!c || (n && (!xyz || !id))) return KS_ERR_INVALID_ARG;
  if (int rc = objects_ready(c, "ks_objects_query")) return rc;
  if (n == 0) return KS_OK;
  if (int rc = quiesce(c)) return rc;
  const size_t m_max = std::min(size_t(1) << 22, n);
  int rc;
  if ((rc = c->obj_out.reserve(c, m_max, m_max))) return rc;
  if ((rc = c->obj_xyz.reserve(c, m_max * 3, m_max * 3))) return rc;
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->obj_xyz, xyz + 3 * off, m * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_obj_query, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, c->stream, c->table, (const uint32_t*)c->obj_ids.get(),
                       c->obj_tiles, (const float*)c->obj_xyz.get(), m, c->voxel_size_inv, c->obj_out.get());
    HIPCHK(c, hipMemcpyAsync(id + off, c->obj_out, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

// ---- navigation field over the stored ESDF ("Navigation field"; ks_k_nav.h) ---------------------
constexpr uint32_t kNavRoundsPerRead = 16;   // rounds enqueued between two host reads of the next list's count

int ks_nav_default_config(ks_nav_config* n) {
  if (!n) return KS_ERR_INVALID_ARG;
  n->radius_m = 0.3f;
  n->max_cost = 0;
  n->max_rounds = 0;
  n->pad = 0;
  return KS_OK;
}

static int nav_refuse(ks_ctx* c, const char* who, const char* why) {
  c->err = std::string(who) + ": " + why;
  return KS_ERR_INVALID_ARG;
}
// what every call asks of the context, then the frames in flight are completed (their statistics stay owed)
static int nav_begin(ks_ctx* c, const char* who) {
  if (int rc = holds_voxels(c, who)) return rc;
  if (c->fatal) return nav_refuse(c, who, "context is in a failed state (earlier pool/index error)");
  return KS_OK;
}
static int nav_read_begin(ks_ctx* c, const char* who) {
  if (int rc = nav_begin(c, who)) return rc;
  if (!c->nav_valid) return nav_refuse(c, who, "no stored field (ks_nav_update has not run since the ESDF store or the map last changed)");
  return quiesce(c);
}
static NavField nav_view(ks_ctx* c) { return NavField{c->nav_cost.get(), c->nav_tiles}; }

int ks_nav_update(ks_ctx* c, const float* goals, size_t n_goals, const ks_nav_config* n, ks_nav_stats* stats) {
  if (!c || !n) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const char* who = "ks_nav_update";
  if (!goals || n_goals < 1 || n_goals > 65536) return nav_refuse(c, who, "goals is NULL or n_goals lies outside 1..65536");
  if (!std::isfinite(n->radius_m) || n->radius_m < 0.0f) return nav_refuse(c, who, "radius_m must be finite and not negative");
  if (n->max_cost > KS_NAV_MAX_COST) return nav_refuse(c, who, "max_cost lies above KS_NAV_MAX_COST");
  if (int rc = nav_begin(c, who)) return rc;
  if (int rc = esdf_ready(c, who)) return rc;
  if (int rc = quiesce(c)) return rc;
  hipStream_t st = c->stream;
  const uint32_t nt = c->esdf_tiles;
  const size_t nvox = (size_t)nt * kTileVoxels;
  const uint32_t max_cost = n->max_cost ? n->max_cost : KS_NAV_MAX_COST, max_rounds = n->max_rounds ? n->max_rounds : 1u << 20;
  int rc;
  c->nav_valid = false;   // (a failure below leaves no field stored)
  if ((rc = c->nav_cost.reserve(c, nvox, ((size_t)nt + nt / 2 + 64) * kTileVoxels)) || (rc = c->nav_lists.reserve(c, 2 * (size_t)nt, 3 * (size_t)nt + 128)) ||
      (rc = c->nav_queued.reserve(c, (size_t)nt + 3, (size_t)nt + nt / 2 + 64)) || (rc = c->nav_counters.reserve(c, 1, 1)) ||
      (rc = c->nav_in.reserve(c, 3 * n_goals, 3 * n_goals)))
    return rc;
  uint32_t* counts = c->nav_queued.get() + nt;
  HIPCHK(c, hipMemsetAsync(c->nav_counters, 0, sizeof(NavCounters), st));
  HIPCHK(c, hipMemsetAsync(c->nav_queued, 0, ((size_t)nt + 3) * sizeof(uint32_t), st));
  HIPCHK(c, hipMemcpyAsync(c->nav_in, goals, 3 * n_goals * sizeof(float), hipMemcpyHostToDevice, st));
  const NavField F{c->nav_cost.get(), nt};
  if (nt)
    hipLaunchKernelGGL(k_nav_init, dim3((uint32_t)((nvox + 255) / 256)), dim3(256), 0, st, (const EsdfRecord*)c->esdf_store.get(), nvox, n->radius_m,
                       c->nav_cost.get(), c->nav_counters.get());
  hipLaunchKernelGGL(k_nav_seed, dim3((uint32_t)((n_goals + 255) / 256)), dim3(256), 0, st, c->table, F, (const float*)c->nav_in.get(), (uint32_t)n_goals,
                     c->voxel_size_inv, c->nav_queued.get(), c->nav_lists.get(), counts, c->nav_counters.get());
  // rounds in groups: the host reads the count of the list the next round would take, once per group
  uint32_t round = 0, active = 0;
  for (;;) {
    HIPCHK(c, hipMemcpyAsync(&active, counts + round % 3u, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (active == 0 || round >= max_rounds) break;
    const uint32_t group = std::min(kNavRoundsPerRead, max_rounds - round);
    for (uint32_t k = 0; k < group; ++k, ++round)
      hipLaunchKernelGGL(k_nav_relax, dim3(nt), dim3(512), 0, st, c->table, F, c->nav_queued.get(), c->nav_lists.get(), counts, round, max_cost,
                         c->nav_counters.get());
  }
  HIPCHK(c, hipGetLastError());
  if (active) {   // a field that has not converged depends on the schedule: none is stored
    c->err = std::string(who) + ": the relaxation is still active after max_rounds = " + std::to_string(max_rounds) + " rounds";
    return KS_ERR_UNSUPPORTED;
  }
  if (nt) hipLaunchKernelGGL(k_nav_count, dim3((uint32_t)((nvox + 255) / 256)), dim3(256), 0, st, (const uint32_t*)c->nav_cost.get(), nvox, c->nav_counters.get());
  NavCounters counters{};
  HIPCHK(c, hipMemcpyAsync(&counters, c->nav_counters, sizeof(counters), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  c->nav_valid = true;
  c->nav_tiles = nt;
  if (stats) {
    stats->voxels_traversable = counters.traversable;
    stats->voxels_reached = counters.reached;
    stats->goals_used = counters.goals_used;
    stats->goals_blocked = counters.goals_blocked;
    stats->largest_cost = counters.largest;
    stats->rounds = counters.rounds;
    stats->tile_relaxations = counters.relaxations;
    stats->workspace_bytes = (uint64_t)nvox * 4 + (uint64_t)nt * 12 + (uint64_t)n_goals * 12;
  }
  return KS_OK;
}

// the field is one word per voxel with all-ones for "nothing here": the readers of the id store (ks_k_nav.h)
static void nav_query_launch(ks_ctx* c, const float* d_xyz, size_t n, uint32_t* d_cost) {
  const size_t per = size_t(1) << 30;
  for (size_t off = 0; off < n; off += per) {
    const size_t m = std::min(per, n - off);
    hipLaunchKernelGGL(k_obj_query, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, c->stream, c->table, (const uint32_t*)c->nav_cost.get(), c->nav_tiles,
                       d_xyz + 3 * off, m, c->voxel_size_inv, d_cost + off);
  }
}

int ks_nav_query_device(ks_ctx* c, const float* d_xyz, size_t n, uint32_t* d_cost) {
  if (!c) return KS_ERR_INVALID_ARG;
  const char* who = "ks_nav_query_device";
  if (n && (!d_xyz || !d_cost)) return nav_refuse(c, who, "xyz or cost is NULL");
  if (int rc = nav_read_begin(c, who)) return rc;
  if (n == 0) return KS_OK;
  nav_query_launch(c, d_xyz, n, d_cost);
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

int ks_nav_query(ks_ctx* c, const float* xyz, size_t n, uint32_t* cost) {
  if (!c) return KS_ERR_INVALID_ARG;
  const char* who = "ks_nav_query";
  if (n && (!xyz || !cost)) return nav_refuse(c, who, "xyz or cost is NULL");
  if (int rc = nav_read_begin(c, who)) return rc;
  if (n == 0) return KS_OK;
  const size_t m_max = std::min(c->nav_chunk, n);
  int rc;
  if ((rc = c->nav_in.reserve(c, 3 * m_max, 3 * m_max)) || (rc = c->nav_u32.reserve(c, m_max, m_max))) return rc;
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->nav_in, xyz + 3 * off, 3 * m * sizeof(float), hipMemcpyHostToDevice, c->stream));
    nav_query_launch(c, c->nav_in, m, c->nav_u32);
    HIPCHK(c, hipMemcpyAsync(cost + off, c->nav_u32, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (the staging is reused by the next chunk)
  }
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

int ks_nav_download_blocks(ks_ctx* c, const int32_t* idx, size_t n, uint32_t* out) {
  if (!c) return KS_ERR_INVALID_ARG;
  const char* who = "ks_nav_download_blocks";
  if (n && (!idx || !out)) return nav_refuse(c, who, "idx_xyz or out is NULL");
  if (int rc = nav_read_begin(c, who)) return rc;
  if (n == 0) return KS_OK;
  const int vps = c->cfg.voxels_per_side;
  const size_t nv = (size_t)vps * vps * vps;
  const size_t chunk = std::min<size_t>(std::max<size_t>(1, (size_t(64) << 20) / (nv * sizeof(uint32_t))), 65535);   // <= 64 MiB staged at a time
  const size_t m_max = std::min(chunk, n);
  int rc;
  if ((rc = c->nav_u32.reserve(c, m_max * nv, m_max * nv)) || (rc = c->nav_idx.reserve(c, m_max * 3, m_max * 3))) return rc;
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->nav_idx, idx + 3 * off, m * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_obj_download, dim3((uint32_t)((nv + 255) / 256), (uint32_t)m), dim3(256), 0, c->stream, c->table,
                       (const uint32_t*)c->nav_cost.get(), c->nav_tiles, (const int32_t*)c->nav_idx.get(), vps, c->nav_u32.get());
    HIPCHK(c, hipMemcpyAsync(out + off * nv, c->nav_u32, m * nv * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

// the checks of both path calls, then the frames in flight are completed and the five counters cleared
static int nav_paths_begin(ks_ctx* c, const char* who, const float* starts, size_t n, uint32_t max_waypoints, bool any_output, ks_nav_path_stats* stats) {
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (max_waypoints < 1 || max_waypoints > 65536) return nav_refuse(c, who, "max_waypoints must lie in 1..65536");
  if (n && !starts) return nav_refuse(c, who, "starts is NULL");
  if (n && !any_output) return nav_refuse(c, who, "all four outputs are NULL");
  if ((uint64_t)n >= (1ull << 32)) return nav_refuse(c, who, "2^32 starts or more in one call");
  if (int rc = nav_read_begin(c, who)) return rc;
  if (int rc = c->nav_path_counters.reserve(c, 8, 8)) return rc;
  HIPCHK(c, hipMemsetAsync(c->nav_path_counters, 0, 8 * sizeof(unsigned long long), c->stream));
  return KS_OK;
}
// k_nav_paths over P.n starts at a DEVICE address (a launch takes at most 2^30 of them)
static void nav_paths_launch(ks_ctx* c, const NavPaths& P) {
  const size_t per = size_t(1) << 30;
  for (size_t off = 0; off < P.n; off += per) {
    NavPaths Q = P;
    Q.n = std::min(per, P.n - off);
    Q.starts += 3 * off;
    if (Q.status) Q.status += off;
    if (Q.cost) Q.cost += off;
    if (Q.n_waypoints) Q.n_waypoints += off;
    if (Q.waypoints) Q.waypoints += off * (size_t)P.max_waypoints * 3;
    hipLaunchKernelGGL(k_nav_paths, dim3((uint32_t)((Q.n + 255) / 256)), dim3(256), 0, c->stream, c->table, nav_view(c), Q);
  }
}
// waits for the stream and reads the five sums
static int nav_paths_stats(ks_ctx* c, ks_nav_path_stats* stats) {
  unsigned long long v[5] = {0, 0, 0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(v, c->nav_path_counters, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  stats->paths_reached = v[0];
  stats->paths_unreachable = v[1];
  stats->paths_blocked = v[2];
  stats->paths_truncated = v[3];
  stats->waypoints = v[4];
  return KS_OK;
}

int ks_nav_paths_device(ks_ctx* c, const float* d_starts, size_t n, uint32_t max_waypoints, uint8_t* d_status, uint32_t* d_cost, uint32_t* d_n_waypoints,
                        float* d_waypoints, ks_nav_path_stats* stats) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (int rc = nav_paths_begin(c, "ks_nav_paths_device", d_starts, n, max_waypoints, d_status || d_cost || d_n_waypoints || d_waypoints, stats)) return rc;
  if (n == 0) return KS_OK;
  nav_paths_launch(c, NavPaths{d_starts, n, max_waypoints, c->cfg.voxel_size, c->voxel_size_inv, d_status, d_cost, d_n_waypoints, d_waypoints,
                               c->nav_path_counters.get()});
  HIPCHK(c, hipGetLastError());
  return stats ? nav_paths_stats(c, stats) : KS_OK;
}

int ks_nav_paths(ks_ctx* c, const float* starts, size_t n, uint32_t max_waypoints, uint8_t* status, uint32_t* cost, uint32_t* n_waypoints, float* waypoints,
                 ks_nav_path_stats* stats) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (int rc = nav_paths_begin(c, "ks_nav_paths", starts, n, max_waypoints, status || cost || n_waypoints || waypoints, stats)) return rc;
  if (n == 0) return KS_OK;
  // a chunk's waypoints stay within 64 MiB; only the rows a path has written reach the caller's array
  const size_t row = (size_t)max_waypoints * 3;
  const size_t m_max = std::min(n, waypoints ? std::min(c->nav_chunk, std::max<size_t>(1, (size_t(64) << 20) / (row * sizeof(float)))) : c->nav_chunk);
  const bool counts = n_waypoints || waypoints;
  int rc;
  if ((rc = c->nav_in.reserve(c, 3 * m_max, 3 * m_max)) || (rc = c->nav_u32.reserve(c, 2 * m_max, 2 * m_max)) || (rc = c->nav_u8.reserve(c, m_max, m_max)) ||
      (waypoints && (rc = c->nav_wp.reserve(c, m_max * row, m_max * row))))
    return rc;
  NavPaths P{c->nav_in.get(), 0, max_waypoints, c->cfg.voxel_size, c->voxel_size_inv, status ? c->nav_u8.get() : nullptr, cost ? c->nav_u32.get() : nullptr,
             counts ? c->nav_u32.get() + m_max : nullptr, waypoints ? c->nav_wp.get() : nullptr, c->nav_path_counters.get()};
  std::vector<uint32_t> nw(counts ? m_max : 0);
  std::vector<float> wp(waypoints ? m_max * row : 0);
  hipStream_t st = c->stream;
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->nav_in, starts + 3 * off, 3 * m * sizeof(float), hipMemcpyHostToDevice, st));
    P.n = m;
    nav_paths_launch(c, P);
    if (status) HIPCHK(c, hipMemcpyAsync(status + off, P.status, m, hipMemcpyDeviceToHost, st));
    if (cost) HIPCHK(c, hipMemcpyAsync(cost + off, P.cost, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (counts) HIPCHK(c, hipMemcpyAsync(nw.data(), P.n_waypoints, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (waypoints) HIPCHK(c, hipMemcpyAsync(wp.data(), P.waypoints, m * row * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));   // (the staging is reused by the next chunk)
    for (size_t i = 0; i < m; ++i) {
      if (n_waypoints) n_waypoints[off + i] = nw[i];
      if (waypoints && nw[i]) std::memcpy(waypoints + (off + i) * row, wp.data() + i * row, (size_t)nw[i] * 3 * sizeof(float));
    }
  }
  HIPCHK(c, hipGetLastError());
  return stats ? nav_paths_stats(c, stats) : KS_OK;
}

// ---- exploration frontiers over the stored ESDF ("Exploration frontiers"; ks_k_frontier.h) -------
int ks_frontiers_default_config(ks_frontier_config* f) {
  if (!f) return KS_ERR_INVALID_ARG;
  std::memset(f, 0, sizeof(*f));
  f->radius_m = 0.3f;
  f->min_voxels = 8;
  return KS_OK;
}

// the work space of an update over nt tiles that finds nc components: per voxel the forest, the ids, the class
// byte and the face count; per tile the two bit planes; per component the accumulator, the record, two keys and three words
static uint64_t frontiers_workspace(uint64_t nt, uint64_t nc) {
  return nt * kTileVoxels * 10 + nt * 128 + sizeof(ObjCounters) + sizeof(FrCounters) + nc * (sizeof(FrAcc) + sizeof(ks_frontier) + 2 * 8 + 3 * 4);
}

int ks_frontiers_update(ks_ctx* c, const ks_frontier_config* f, ks_frontier_stats* stats) {
  if (!c || !f) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const char* who = "ks_frontiers_update";
  if (!std::isfinite(f->radius_m) || f->radius_m < 0.0f) return nav_refuse(c, who, "radius_m must be finite and not negative");
  if (f->min_voxels < 1) return nav_refuse(c, who, "min_voxels must be at least 1");
  if (f->use_bounds)
    for (int k = 0; k < 3; ++k)
      if (f->bounds_min[k] > f->bounds_max[k]) return nav_refuse(c, who, "a bounds_min lies above its bounds_max");
  if (int rc = nav_begin(c, who)) return rc;
  if (int rc = esdf_ready(c, who)) return rc;
  if (int rc = quiesce(c)) return rc;
  hipStream_t st = c->stream;
  const uint32_t nt = c->esdf_tiles;
  if (nt >= (1u << 23)) {   // (a voxel's id is slot * 512 + local in 32 bits, all-ones = none)
    c->err = std::string(who) + ": too many tiles for one call";
    return KS_ERR_UNSUPPORTED;
  }
  const size_t nvox = (size_t)nt * kTileVoxels;
  const bool with_field = c->nav_valid && c->nav_tiles == nt;   // (a stored field is a snapshot of this same store)
  int rc;
  drop_frontiers(c);   // (a failure below leaves nothing stored)
  if ((rc = c->fr_ids.reserve(c, nvox, ((size_t)nt + nt / 2 + 64) * kTileVoxels)) || (rc = c->fr_parent.reserve(c, nvox, nvox + nvox / 2)) ||
      (rc = c->fr_cls.reserve(c, nvox, nvox + nvox / 2)) || (rc = c->fr_faces.reserve(c, nvox, nvox + nvox / 2)) ||
      (rc = c->fr_planes.reserve(c, (size_t)nt * 16, ((size_t)nt + nt / 2) * 16)) || (rc = c->fr_numbered.reserve(c, 1, 1)) ||
      (rc = c->fr_counters.reserve(c, 1, 1)))
    return rc;
  HIPCHK(c, hipMemsetAsync(c->fr_numbered, 0, sizeof(ObjCounters), st));
  HIPCHK(c, hipMemsetAsync(c->fr_counters, 0, sizeof(FrCounters), st));
  FrParams F{};
  F.radius = f->radius_m;
  F.min_voxels = f->min_voxels;
  F.use_bounds = f->use_bounds ? 1 : 0;
  for (int k = 0; k < 3; ++k) F.bmin[k] = f->bounds_min[k], F.bmax[k] = f->bounds_max[k];
  F.nt = nt;
  ObjParams O{};   // (k_obj_seams reads the tile count alone)
  O.nt = nt;
  ObjCounters numbered{};
  FrCounters counts{};
  if (nt) {
    // 1) the bit planes, the classes and the in-tile forest; seams, flat forest and provisional numbers as the objects do
    hipLaunchKernelGGL(k_fr_planes, dim3(nt * 2), dim3(256), 0, st, c->table, F, (const EsdfRecord*)c->esdf_store.get(), c->fr_planes.get(),
                       c->fr_counters.get());
    hipLaunchKernelGGL(k_fr_classify, dim3(nt), dim3(512), 0, st, c->table, F, (const unsigned long long*)c->fr_planes.get(), c->fr_cls.get(),
                       c->fr_faces.get(), c->fr_parent.get(), c->fr_counters.get());
    hipLaunchKernelGGL(k_obj_seams, dim3(nt), dim3(512), 0, st, c->table, O, (const uint8_t*)c->fr_cls.get(), c->fr_parent.get());
    hipLaunchKernelGGL(k_obj_number, dim3(nt * 2), dim3(256), 0, st, c->fr_parent.get(), c->fr_ids.get(), c->fr_numbered.get());
    HIPCHK(c, hipMemcpyAsync(&numbered, c->fr_numbered, sizeof(numbered), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));   // the one read that sizes what follows
    const uint32_t nc = numbered.n_components;
    if (nc) {
      // 2) reduce, join with the field, filter, order, assign
      const size_t cap = (size_t)nc + nc / 2;
      if ((rc = c->fr_acc.reserve(c, nc, cap)) || (rc = c->fr_final.reserve(c, nc, cap)) || (rc = c->fr_records.reserve(c, nc, cap))) return rc;
      for (int k = 0; k < 2; ++k)
        if ((rc = c->fr_keys[k].reserve(c, nc, cap)) || (rc = c->fr_vals[k].reserve(c, nc, cap))) return rc;
      const dim3 per_comp((nc + 255) / 256);
      const uint32_t* field = with_field ? (const uint32_t*)c->nav_cost.get() : nullptr;
      hipLaunchKernelGGL(k_fr_acc_init, per_comp, dim3(256), 0, st, c->fr_acc.get(), nc);
      hipLaunchKernelGGL(k_fr_reduce, dim3(nt * 2), dim3(256), 0, st, c->table, (const uint8_t*)c->fr_faces.get(), field, c->fr_parent.get(),
                         (const uint32_t*)c->fr_ids.get(), c->fr_acc.get());
      if (field)
        hipLaunchKernelGGL(k_fr_nav_pick, dim3(nt * 2), dim3(256), 0, st, c->table, field, (const uint32_t*)c->fr_parent.get(), c->fr_acc.get());
      hipLaunchKernelGGL(k_fr_keys, per_comp, dim3(256), 0, st, (const FrAcc*)c->fr_acc.get(), nc, F.min_voxels, c->fr_keys[0].get(),
                         c->fr_vals[0].get(), c->fr_counters.get());
      uint64_t* keys = nullptr;
      uint32_t* vals = nullptr;
      if ((rc = sort_pairs(c, c->fr_keys[0].get(), c->fr_keys[1].get(), c->fr_vals[0].get(), c->fr_vals[1].get(), nc, 64, &keys, &vals))) return rc;
      hipLaunchKernelGGL(k_fr_records, per_comp, dim3(256), 0, st, (const FrAcc*)c->fr_acc.get(), nc, (const uint64_t*)keys, (const uint32_t*)vals,
                         c->fr_records.get(), c->fr_final.get());
    }
    hipLaunchKernelGGL(k_obj_ids, dim3((uint32_t)((nvox + 255) / 256)), dim3(256), 0, st, (const uint32_t*)c->fr_parent.get(),
                       (const uint32_t*)c->fr_final.get(), c->fr_ids.get(), nvox);
    HIPCHK(c, hipMemcpyAsync(&counts, c->fr_counters, sizeof(counts), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  c->fr_valid = true;
  c->fr_tiles = nt;
  c->fr_count = counts.n_frontiers;
  if (stats) {
    stats->voxels_traversable = counts.traversable;
    stats->voxels_frontier = counts.frontier_voxels;
    stats->components = numbered.n_components;
    stats->frontiers = counts.n_frontiers;
    stats->voxels_in_frontiers = counts.voxels_in_frontiers;
    stats->largest_frontier_voxels = counts.largest;
    stats->unknown_faces = counts.unknown_faces;
    stats->nav_field_used = with_field ? 1 : 0;
    stats->workspace_bytes = frontiers_workspace(nt, numbered.n_components);
  }
  return KS_OK;
}

static int frontiers_read_begin(ks_ctx* c, const char* who) {
  if (int rc = nav_begin(c, who)) return rc;
  if (!c->fr_valid)
    return nav_refuse(c, who, "no frontiers are stored (ks_frontiers_update has not run since the ESDF store or the map last changed)");
  return KS_OK;
}

int ks_frontiers_size(ks_ctx* c, size_t* n) {
  if (!c || !n) return KS_ERR_INVALID_ARG;
  if (int rc = frontiers_read_begin(c, "ks_frontiers_size")) return rc;
  *n = c->fr_count;
  return KS_OK;
}

int ks_frontiers_download(ks_ctx* c, ks_frontier* out, size_t cap, size_t* n) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (int rc = frontiers_read_begin(c, "ks_frontiers_download")) return rc;
  if (n) *n = c->fr_count;
  if (cap < c->fr_count || (c->fr_count && !out)) return nav_refuse(c, "ks_frontiers_download", "output buffer too small");
  if (c->fr_count) HIPCHK(c, hipMemcpy(out, c->fr_records.get(), c->fr_count * sizeof(ks_frontier), hipMemcpyDeviceToHost));
  return KS_OK;
}

int ks_frontiers_download_blocks(ks_ctx* c, const int32_t* idx, size_t n, uint32_t* out) {
  if (!c) return KS_ERR_INVALID_ARG;
  const char* who = "ks_frontiers_download_blocks";
  if (n && (!idx || !out)) return nav_refuse(c, who, "block_idx_xyz or out is NULL");
  if (int rc = frontiers_read_begin(c, who)) return rc;
  if (n == 0) return KS_OK;
  if (int rc = quiesce(c)) return rc;
  const int vps = c->cfg.voxels_per_side;
  const size_t nv = (size_t)vps * vps * vps;
  const size_t chunk = std::min<size_t>(std::max<size_t>(1, (size_t(64) << 20) / (nv * sizeof(uint32_t))), 65535);   // <= 64 MiB staged at a time
  const size_t m_max = std::min(chunk, n);
  int rc;
  if ((rc = c->fr_out.reserve(c, m_max * nv, m_max * nv)) || (rc = c->fr_idx.reserve(c, m_max * 3, m_max * 3))) return rc;
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->fr_idx, idx + 3 * off, m * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_obj_download, dim3((uint32_t)((nv + 255) / 256), (uint32_t)m), dim3(256), 0, c->stream, c->table,
                       (const uint32_t*)c->fr_ids.get(), c->fr_tiles, (const int32_t*)c->fr_idx.get(), vps, c->fr_out.get());
    HIPCHK(c, hipMemcpyAsync(out + off * nv, c->fr_out, m * nv * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

int ks_frontiers_query(ks_ctx* c, const float* xyz, size_t n, uint32_t* id) {
  if (!c) return KS_ERR_INVALID_ARG;
  const char* who = "ks_frontiers_query";
  if (n && (!xyz || !id)) return nav_refuse(c, who, "xyz or id is NULL");
  if (int rc = frontiers_read_begin(c, who)) return rc;
  if (n == 0) return KS_OK;
  if (int rc = quiesce(c)) return rc;
  const size_t m_max = std::min(size_t(1) << 22, n);
  int rc;
  if ((rc = c->fr_out.reserve(c, m_max, m_max)) || (rc = c->fr_xyz.reserve(c, m_max * 3, m_max * 3))) return rc;
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->fr_xyz, xyz + 3 * off, m * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_obj_query, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, c->stream, c->table, (const uint32_t*)c->fr_ids.get(),
                       c->fr_tiles, (const float*)c->fr_xyz.get(), m, c->voxel_size_inv, c->fr_out.get());
    HIPCHK(c, hipMemcpyAsync(id + off, c->fr_out, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

// ---- rooms over the stored ESDF ("Rooms"; ks_k_rooms.h) -------
int ks_rooms_default_config(ks_rooms_config* r) {
  if (!r) return KS_ERR_INVALID_ARG;
  std::memset(r, 0, sizeof(*r));
  r->core_distance_m = 0.5f;
  r->min_core_voxels = 64;
  return KS_OK;
}

// the work space of an update over nt tiles that finds nc core components, np contact pairs, nl links and joins no objects
// (DESIGN.md §25.2): per voxel the two planes, the forest and the class byte; per tile two list entries and the queued flag; per
// component what the objects keep (accumulator, record, two keys, three words) plus the room's accumulator and record; per pair two
// keys and two words, and as much for the heads (a pair may be one); per link its accumulator and its record; per object its key
// and its room
static uint64_t rooms_workspace(uint64_t nt, uint64_t nc, uint64_t np, uint64_t nl, uint64_t no) {
  return nt * kTileVoxels * 13 + nt * 12 + 12 + sizeof(ObjCounters) + sizeof(NavCounters) + sizeof(RoomCounters) +
         nc * (sizeof(ObjAcc) + sizeof(ks_object) + 2 * 8 + 3 * 4 + sizeof(RoomAcc) + sizeof(ks_room)) + np * 2 * (2 * 8 + 2 * 4) +
         nl * (sizeof(RoomLinkAcc) + sizeof(ks_room_link)) + no * (8 + 4);
}

// One of the two relaxations of ks_rooms_update: list 0 holds the seeded tiles; rounds in groups as in ks_nav_update.  *active is
// what the next round would take when the loop ends: not 0 after max_rounds rounds.
extern "C++" template <class Launch>
static int rooms_relax(ks_ctx* c, uint32_t* counts, uint32_t max_rounds, uint32_t* active, Launch launch) {
  hipStream_t st = c->stream;
  uint32_t round = 0;
  for (;;) {
    HIPCHK(c, hipMemcpyAsync(active, counts + round % 3u, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (*active == 0 || round >= max_rounds) break;
    const uint32_t group = std::min(kNavRoundsPerRead, max_rounds - round);
    for (uint32_t k = 0; k < group; ++k, ++round) launch(round);
  }
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

int ks_rooms_update(ks_ctx* c, const ks_rooms_config* r, ks_rooms_stats* stats) {
  if (!c || !r) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const char* who = "ks_rooms_update";
  if (!std::isfinite(r->free_distance_m) || r->free_distance_m < 0.0f) return nav_refuse(c, who, "free_distance_m must be finite and not negative");
  if (!std::isfinite(r->core_distance_m) || r->core_distance_m < 0.0f) return nav_refuse(c, who, "core_distance_m must be finite and not negative");
  if (r->core_distance_m < r->free_distance_m) return nav_refuse(c, who, "core_distance_m lies below free_distance_m");
  if (r->min_core_voxels < 1) return nav_refuse(c, who, "min_core_voxels must be at least 1");
  if (r->max_cost > KS_NAV_MAX_COST) return nav_refuse(c, who, "max_cost lies above KS_NAV_MAX_COST");
  if (r->use_bounds)
    for (int k = 0; k < 3; ++k)
      if (r->bounds_min[k] > r->bounds_max[k]) return nav_refuse(c, who, "a bounds_min lies above its bounds_max");
  if (int rc = nav_begin(c, who)) return rc;
  if (int rc = esdf_ready(c, who)) return rc;
  if (int rc = quiesce(c)) return rc;
  hipStream_t st = c->stream;
  const uint32_t nt = c->esdf_tiles;
  if (nt >= (1u << 23)) {   // (a voxel's id is slot * 512 + local in 32 bits, all-ones = none)
    c->err = std::string(who) + ": too many tiles for one call";
    return KS_ERR_UNSUPPORTED;
  }
  const size_t nvox = (size_t)nt * kTileVoxels;
  const uint32_t max_cost = r->max_cost ? r->max_cost : KS_NAV_MAX_COST, max_rounds = r->max_rounds ? r->max_rounds : 1u << 20;
  // the objects as they are stored now: their ids in the slots both stores cover (a later ks_objects_update is not seen)
  const uint32_t n_obj = c->obj_valid ? (uint32_t)c->obj_count : 0u;
  const size_t obj_vox = (size_t)std::min(c->obj_tiles, nt) * kTileVoxels;
  int rc;
  drop_rooms(c);   // (a failure below leaves nothing stored)
  const size_t vox_cap = ((size_t)nt + nt / 2 + 64) * kTileVoxels;
  if ((rc = c->rooms_room.reserve(c, nvox, vox_cap)) || (rc = c->rooms_cost.reserve(c, nvox, vox_cap)) || (rc = c->rooms_parent.reserve(c, nvox, nvox + nvox / 2)) ||
      (rc = c->rooms_cls.reserve(c, nvox, nvox + nvox / 2)) || (rc = c->rooms_lists.reserve(c, 2 * (size_t)nt, 3 * (size_t)nt + 128)) ||
      (rc = c->rooms_queued.reserve(c, (size_t)nt + 3, (size_t)nt + nt / 2 + 64)) || (rc = c->rooms_nav_counters.reserve(c, 1, 1)) ||
      (rc = c->rooms_numbered.reserve(c, 1, 1)) || (rc = c->rooms_counters.reserve(c, 1, 1)) || (rc = c->rooms_obj_room.reserve(c, n_obj, n_obj)) ||
      (rc = c->rooms_obj_best.reserve(c, n_obj, n_obj)))
    return rc;
  uint32_t* counts = c->rooms_queued.get() + nt;
  HIPCHK(c, hipMemsetAsync(c->rooms_nav_counters, 0, sizeof(NavCounters), st));
  HIPCHK(c, hipMemsetAsync(c->rooms_numbered, 0, sizeof(ObjCounters), st));
  HIPCHK(c, hipMemsetAsync(c->rooms_counters, 0, sizeof(RoomCounters), st));
  HIPCHK(c, hipMemsetAsync(c->rooms_queued, 0, ((size_t)nt + 3) * sizeof(uint32_t), st));
  if (n_obj) HIPCHK(c, hipMemsetAsync(c->rooms_obj_room, 0xff, (size_t)n_obj * sizeof(uint32_t), st));
  RoomParams R{};
  R.free_distance = r->free_distance_m;
  R.core_distance = r->core_distance_m;
  R.use_bounds = r->use_bounds ? 1 : 0;
  for (int k = 0; k < 3; ++k) R.bmin[k] = r->bounds_min[k], R.bmax[k] = r->bounds_max[k];
  R.nt = nt;
  ObjParams O{};   // (k_obj_seams reads the tile count alone)
  O.nt = nt;
  ObjCounters numbered{};
  RoomCounters counts_h{};
  NavCounters relax_h{};
  uint32_t nc = 0, n_rooms = 0, n_pairs = 0, n_links = 0;
  const EsdfRecord* store = (const EsdfRecord*)c->esdf_store.get();
  const NavField F{c->rooms_cost.get(), nt};
  if (nt) {
    // 1) classes, initial costs, the core components: seams, flat forest and provisional numbers as the objects do
    hipLaunchKernelGGL(k_room_classify, dim3(nt), dim3(512), 0, st, c->table, R, store, c->rooms_cls.get(), c->rooms_parent.get(), c->rooms_cost.get(),
                       c->rooms_counters.get());
    hipLaunchKernelGGL(k_obj_seams, dim3(nt), dim3(512), 0, st, c->table, O, (const uint8_t*)c->rooms_cls.get(), c->rooms_parent.get());
    hipLaunchKernelGGL(k_obj_number, dim3(nt * 2), dim3(256), 0, st, c->rooms_parent.get(), c->rooms_room.get(), c->rooms_numbered.get());
    HIPCHK(c, hipMemcpyAsync(&numbered, c->rooms_numbered, sizeof(numbered), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));   // the read that sizes the component buffers
    nc = numbered.n_components;
  }
  if (nc) {
    // 2) the components' sizes and smallest voxels, the filter, the order: provisional number -> room
    const size_t cap = (size_t)nc + nc / 2;
    if ((rc = c->rooms_core_acc.reserve(c, nc, cap)) || (rc = c->rooms_final.reserve(c, nc, cap)) || (rc = c->rooms_cores.reserve(c, nc, cap)) ||
        (rc = c->rooms_acc.reserve(c, nc, cap)) || (rc = c->rooms_records.reserve(c, nc, cap)))
      return rc;
    for (int k = 0; k < 2; ++k)
      if ((rc = c->rooms_keys[k].reserve(c, nc, cap)) || (rc = c->rooms_vals[k].reserve(c, nc, cap))) return rc;
    const dim3 per_comp((nc + 255) / 256);
    hipLaunchKernelGGL(k_obj_acc_init, per_comp, dim3(256), 0, st, c->rooms_core_acc.get(), nc);
    hipLaunchKernelGGL(k_obj_reduce, dim3(nt * 2), dim3(256), 0, st, c->table, (const uint8_t*)c->rooms_cls.get(), c->rooms_parent.get(),
                       (const uint32_t*)c->rooms_room.get(), c->rooms_core_acc.get());
    hipLaunchKernelGGL(k_obj_keys, per_comp, dim3(256), 0, st, (const ObjAcc*)c->rooms_core_acc.get(), nc, r->min_core_voxels, c->rooms_keys[0].get(),
                       c->rooms_vals[0].get(), c->rooms_numbered.get());
    uint64_t* keys = nullptr;
    uint32_t* vals = nullptr;
    if ((rc = sort_pairs(c, c->rooms_keys[0].get(), c->rooms_keys[1].get(), c->rooms_vals[0].get(), c->rooms_vals[1].get(), nc, 64, &keys, &vals))) return rc;
    hipLaunchKernelGGL(k_obj_records, per_comp, dim3(256), 0, st, (const ObjAcc*)c->rooms_core_acc.get(), nc, (const uint64_t*)keys, (const uint32_t*)vals,
                       c->rooms_cores.get(), c->rooms_final.get());
    hipLaunchKernelGGL(k_room_acc_init, per_comp, dim3(256), 0, st, c->rooms_acc.get(), nc);
    // 3) the multi-source cost: k_nav_relax from the cores of the rooms
    hipLaunchKernelGGL(k_room_seed, dim3(nt * 2), dim3(256), 0, st, (const uint32_t*)c->rooms_parent.get(), (const uint32_t*)c->rooms_final.get(), 1,
                       c->rooms_room.get(), c->rooms_cost.get(), c->rooms_queued.get(), c->rooms_lists.get(), counts);
    uint32_t active = 0;
    if ((rc = rooms_relax(c, counts, max_rounds, &active, [&](uint32_t round) {
           hipLaunchKernelGGL(k_nav_relax, dim3(nt), dim3(512), 0, st, c->table, F, c->rooms_queued.get(), c->rooms_lists.get(), counts, round, max_cost,
                              c->rooms_nav_counters.get());
         })))
      return rc;
    if (!active) {
      // 4) the room of every reached voxel, down the shortest-path graph from the same seeds
      HIPCHK(c, hipMemsetAsync(c->rooms_queued, 0, ((size_t)nt + 3) * sizeof(uint32_t), st));
      hipLaunchKernelGGL(k_room_seed, dim3(nt * 2), dim3(256), 0, st, (const uint32_t*)c->rooms_parent.get(), (const uint32_t*)c->rooms_final.get(), 0,
                         c->rooms_room.get(), c->rooms_cost.get(), c->rooms_queued.get(), c->rooms_lists.get(), counts);
      if ((rc = rooms_relax(c, counts, max_rounds, &active, [&](uint32_t round) {
             hipLaunchKernelGGL(k_room_assign, dim3(nt), dim3(512), 0, st, c->table, F, c->rooms_room.get(), c->rooms_queued.get(), c->rooms_lists.get(), counts,
                                round, c->rooms_nav_counters.get());
           })))
        return rc;
    }
    if (active) {   // a result that has not converged depends on the schedule: none is stored
      c->err = std::string(who) + ": a relaxation is still active after max_rounds = " + std::to_string(max_rounds) + " rounds";
      return KS_ERR_UNSUPPORTED;
    }
    // 5) per room: the assigned voxels, the clearance and where it is attained
    hipLaunchKernelGGL(k_room_reduce, dim3(nt * 2), dim3(256), 0, st, c->table, store, (const uint32_t*)c->rooms_room.get(),
                       (const uint32_t*)c->rooms_cost.get(), c->rooms_acc.get());
    hipLaunchKernelGGL(k_room_pick, dim3(nt * 2), dim3(256), 0, st, c->table, store, (const uint32_t*)c->rooms_room.get(), (const uint32_t*)c->rooms_cost.get(),
                       c->rooms_acc.get());
    // 6) the contacts: counted, emitted, sorted; the heads of the runs are the links
    RoomCounters* C = c->rooms_counters.get();
    hipLaunchKernelGGL(k_room_contacts, dim3(nt), dim3(512), 0, st, c->table, nt, (const uint32_t*)c->rooms_room.get(), 0, &C->n_pairs, (uint64_t*)nullptr,
                       (uint32_t*)nullptr);
    HIPCHK(c, hipMemcpyAsync(&numbered, c->rooms_numbered, sizeof(numbered), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&counts_h, c->rooms_counters, sizeof(counts_h), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));   // the read that sizes the pair buffers
    n_rooms = numbered.n_objects;
    n_pairs = counts_h.n_pairs;
    if (n_pairs >= (1u << 31)) {
      c->err = std::string(who) + ": too many contacts for one call";
      return KS_ERR_UNSUPPORTED;
    }
    if (n_pairs) {
      const size_t pcap = (size_t)n_pairs + n_pairs / 2;
      for (int k = 0; k < 2; ++k)
        if ((rc = c->rooms_keys[k].reserve(c, n_pairs, pcap)) || (rc = c->rooms_vals[k].reserve(c, n_pairs, pcap)) ||
            (rc = c->rooms_head_keys[k].reserve(c, n_pairs, pcap)) || (rc = c->rooms_head_vals[k].reserve(c, n_pairs, pcap)))
          return rc;
      hipLaunchKernelGGL(k_room_contacts, dim3(nt), dim3(512), 0, st, c->table, nt, (const uint32_t*)c->rooms_room.get(), 1, &C->cursor, c->rooms_keys[0].get(),
                         c->rooms_vals[0].get());
      const unsigned key_bits = 32 + bits_for(n_rooms);
      if ((rc = sort_pairs(c, c->rooms_keys[0].get(), c->rooms_keys[1].get(), c->rooms_vals[0].get(), c->rooms_vals[1].get(), n_pairs, key_bits, &keys, &vals))) return rc;
      hipLaunchKernelGGL(k_room_heads, dim3((n_pairs + 255) / 256), dim3(256), 0, st, (const uint64_t*)keys, n_pairs, c->rooms_head_keys[0].get(),
                         c->rooms_head_vals[0].get(), &C->n_links);
      HIPCHK(c, hipMemcpyAsync(&counts_h, c->rooms_counters, sizeof(counts_h), hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));   // the read that sizes the link buffers
      n_links = counts_h.n_links;
      uint64_t* head_keys = nullptr;
      uint32_t* starts = nullptr;
      if ((rc = c->rooms_link_acc.reserve(c, n_links, n_links + n_links / 2)) || (rc = c->rooms_links.reserve(c, n_links, n_links + n_links / 2)) ||
          (rc = sort_pairs(c, c->rooms_head_keys[0].get(), c->rooms_head_keys[1].get(), c->rooms_head_vals[0].get(), c->rooms_head_vals[1].get(), n_links, key_bits,
                           &head_keys, &starts)))
        return rc;
      const dim3 per_pair((n_pairs + 255) / 256), per_link((n_links + 255) / 256);
      hipLaunchKernelGGL(k_room_link_init, per_link, dim3(256), 0, st, c->rooms_link_acc.get(), n_links);
      hipLaunchKernelGGL(k_room_link_max, per_pair, dim3(256), 0, st, store, (const uint32_t*)vals, n_pairs, (const uint32_t*)starts, n_links,
                         c->rooms_link_acc.get());
      hipLaunchKernelGGL(k_room_link_pick, per_pair, dim3(256), 0, st, c->table, store, (const uint32_t*)vals, n_pairs, (const uint32_t*)starts, n_links,
                         c->rooms_link_acc.get());
      hipLaunchKernelGGL(k_room_links, per_link, dim3(256), 0, st, c->table, nt, (const uint32_t*)c->rooms_room.get(), (const uint64_t*)head_keys,
                         (const uint32_t*)starts, n_links, n_pairs, (const RoomLinkAcc*)c->rooms_link_acc.get(), c->rooms_acc.get(), c->rooms_links.get());
    }
    // 7) the join with the stored objects
    if (n_obj && n_rooms) {
      HIPCHK(c, hipMemsetAsync(c->rooms_obj_best, 0xff, (size_t)n_obj * sizeof(unsigned long long), st));
      if (obj_vox)
        hipLaunchKernelGGL(k_room_obj_min, dim3((uint32_t)((obj_vox + 255) / 256)), dim3(256), 0, st, (const uint32_t*)c->obj_ids.get(), n_obj,
                           (const uint32_t*)c->rooms_room.get(), (const uint32_t*)c->rooms_cost.get(), obj_vox, c->rooms_obj_best.get());
      hipLaunchKernelGGL(k_room_obj_join, dim3((n_obj + 255) / 256), dim3(256), 0, st, (const unsigned long long*)c->rooms_obj_best.get(), n_obj,
                         c->rooms_obj_room.get(), c->rooms_acc.get(), c->rooms_counters.get());
    }
    // 8) the records
    if (n_rooms)
      hipLaunchKernelGGL(k_room_records, dim3((n_rooms + 255) / 256), dim3(256), 0, st, (const ks_object*)c->rooms_cores.get(), (const RoomAcc*)c->rooms_acc.get(),
                         n_rooms, c->rooms_records.get(), c->rooms_counters.get());
  } else if (nt) {
    HIPCHK(c, hipMemsetAsync(c->rooms_room, 0xff, nvox * sizeof(uint32_t), st));   // no core voxel: no room, nothing assigned
  }
  HIPCHK(c, hipMemcpyAsync(&counts_h, c->rooms_counters, sizeof(counts_h), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(&relax_h, c->rooms_nav_counters, sizeof(relax_h), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  c->rooms_valid = true;
  c->rooms_tiles = nt;
  c->rooms_count = n_rooms;
  c->rooms_link_count = n_links;
  c->rooms_obj_count = n_obj;
  if (stats) {
    stats->voxels_free = counts_h.free_voxels;
    stats->voxels_core = counts_h.core_voxels;
    stats->components = nc;
    stats->rooms = n_rooms;
    stats->voxels_assigned = counts_h.assigned;
    stats->voxels_unassigned = counts_h.free_voxels - counts_h.assigned;
    stats->largest_room_voxels = counts_h.largest_room;
    stats->largest_cost = counts_h.largest_cost;
    stats->links = n_links;
    stats->contacts = n_pairs;
    stats->objects_seen = n_obj;
    stats->objects_joined = counts_h.objects_joined;
    stats->rounds = relax_h.rounds;
    stats->tile_relaxations = relax_h.relaxations;
    stats->workspace_bytes = rooms_workspace(nt, nc, n_pairs, n_links, n_obj);
  }
  return KS_OK;
}

static int rooms_read_begin(ks_ctx* c, const char* who) {
  if (int rc = nav_begin(c, who)) return rc;
  if (!c->rooms_valid) return nav_refuse(c, who, "no rooms are stored (ks_rooms_update has not run since the ESDF store or the map last changed)");
  return KS_OK;
}

int ks_rooms_size(ks_ctx* c, size_t* n_rooms, size_t* n_links) {
  if (!c || (!n_rooms && !n_links)) return KS_ERR_INVALID_ARG;
  if (int rc = rooms_read_begin(c, "ks_rooms_size")) return rc;
  if (n_rooms) *n_rooms = c->rooms_count;
  if (n_links) *n_links = c->rooms_link_count;
  return KS_OK;
}

// the download of one of the three lists: *n receives the count, cap must hold it
extern "C++" template <class T>
static int rooms_list(ks_ctx* c, const char* who, const T* d_list, size_t count, T* out, size_t cap, size_t* n) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (int rc = rooms_read_begin(c, who)) return rc;
  if (n) *n = count;
  if (cap < count || (count && !out)) return nav_refuse(c, who, "output buffer too small");
  if (count) HIPCHK(c, hipMemcpy(out, d_list, count * sizeof(T), hipMemcpyDeviceToHost));
  return KS_OK;
}

int ks_rooms_download(ks_ctx* c, ks_room* out, size_t cap, size_t* n) {
  return rooms_list(c, "ks_rooms_download", c ? (const ks_room*)c->rooms_records.get() : nullptr, c ? c->rooms_count : 0, out, cap, n);
}

int ks_rooms_links_download(ks_ctx* c, ks_room_link* out, size_t cap, size_t* n) {
  return rooms_list(c, "ks_rooms_links_download", c ? (const ks_room_link*)c->rooms_links.get() : nullptr, c ? c->rooms_link_count : 0, out, cap, n);
}

int ks_rooms_objects(ks_ctx* c, uint32_t* room_of_object, size_t cap, size_t* n) {
  return rooms_list(c, "ks_rooms_objects", c ? (const uint32_t*)c->rooms_obj_room.get() : nullptr, c ? c->rooms_obj_count : 0, room_of_object, cap, n);
}

int ks_rooms_download_blocks(ks_ctx* c, const int32_t* idx, size_t n, uint32_t* room, uint32_t* cost) {
  if (!c) return KS_ERR_INVALID_ARG;
  const char* who = "ks_rooms_download_blocks";
  if (n && (!idx || (!room && !cost))) return nav_refuse(c, who, "block_idx_xyz is NULL, or both room and cost are");
  if (int rc = rooms_read_begin(c, who)) return rc;
  if (n == 0) return KS_OK;
  if (int rc = quiesce(c)) return rc;
  const int vps = c->cfg.voxels_per_side;
  const size_t nv = (size_t)vps * vps * vps;
  const size_t chunk = std::min<size_t>(std::max<size_t>(1, (size_t(64) << 20) / (nv * sizeof(uint32_t))), 65535);   // <= 64 MiB staged at a time
  const size_t m_max = std::min(chunk, n);
  int rc;
  if ((rc = c->rooms_out.reserve(c, m_max * nv, m_max * nv)) || (rc = c->rooms_idx.reserve(c, m_max * 3, m_max * 3))) return rc;
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->rooms_idx, idx + 3 * off, m * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    for (int plane = 0; plane < 2; ++plane) {
      uint32_t* out = plane ? cost : room;
      if (!out) continue;
      hipLaunchKernelGGL(k_obj_download, dim3((uint32_t)((nv + 255) / 256), (uint32_t)m), dim3(256), 0, c->stream, c->table,
                         (const uint32_t*)(plane ? c->rooms_cost.get() : c->rooms_room.get()), c->rooms_tiles, (const int32_t*)c->rooms_idx.get(), vps, c->rooms_out.get());
      HIPCHK(c, hipMemcpyAsync(out + off * nv, c->rooms_out, m * nv * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));   // (the staging is reused by the next plane and the next chunk)
    }
  }
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

int ks_rooms_query(ks_ctx* c, const float* xyz, size_t n, uint32_t* room) {
  if (!c) return KS_ERR_INVALID_ARG;
  const char* who = "ks_rooms_query";
  if (n && (!xyz || !room)) return nav_refuse(c, who, "xyz or room is NULL");
  if (int rc = rooms_read_begin(c, who)) return rc;
  if (n == 0) return KS_OK;
  if (int rc = quiesce(c)) return rc;
  const size_t m_max = std::min(size_t(1) << 22, n);
  int rc;
  if ((rc = c->rooms_out.reserve(c, m_max, m_max)) || (rc = c->rooms_xyz.reserve(c, m_max * 3, m_max * 3))) return rc;
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->rooms_xyz, xyz + 3 * off, m * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_obj_query, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, c->stream, c->table, (const uint32_t*)c->rooms_room.get(), c->rooms_tiles,
                       (const float*)c->rooms_xyz.get(), m, c->voxel_size_inv, c->rooms_out.get());
    HIPCHK(c, hipMemcpyAsync(room + off, c->rooms_out, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

// ---- view information gain over the stored ESDF ("View information gain"; ks_k_view_gain.h) -------
int ks_view_gain_default_config(ks_view_gain_config* g) {
  if (!g) return KS_ERR_INVALID_ARG;
  std::memset(g, 0, sizeof(*g));
  g->max_range_m = 5.0f;
  g->width = 32;
  g->height = 24;
  g->label = 255;
  g->max_workspace_bytes = uint64_t(1) << 30;
  return KS_OK;
}

// the checks of both calls and the sizing rule of DESIGN.md §22.2, then both kernels on the context's stream: DEVICE records out;
// the poses are DEVICE memory, or with `staged` host memory that goes through the context's staging (the records then land in
// c->vg_records).  The host is not waited for here.  *launched = false: nothing to do (n = 0).
static int view_gain_enqueue(ks_ctx* c, const char* who, const float* poses, bool staged, size_t n, const ks_view_gain_config* g,
                             ks_view_gain_record* d_out, ks_view_gain_stats* stats, bool* launched) {
  *launched = false;
  if (n && (!poses || !d_out)) return nav_refuse(c, who, "T_G_C or out is NULL");
  if (g->width < 1 || g->width > 1024 || g->height < 1 || g->height > 1024 || g->width * g->height > 65536)
    return nav_refuse(c, who, "width and height must lie in 1..1024 and width * height in 1..65536");
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(g->K[k])) return nav_refuse(c, who, "K must be finite");
  if (!(g->K[0] > 0.0f) || !(g->K[1] > 0.0f)) return nav_refuse(c, who, "fx and fy must be positive");
  const float par[4] = {g->min_range_m, g->max_range_m, g->step_m, g->stop_distance_m};
  for (float v : par)
    if (!std::isfinite(v) || v < 0.0f) return nav_refuse(c, who, "min_range_m, max_range_m, step_m and stop_distance_m must be finite and not negative");
  if (g->min_range_m > g->max_range_m) return nav_refuse(c, who, "min_range_m lies above max_range_m");
  if (g->label > 255) return nav_refuse(c, who, "label lies above 255");
  if (n >= (size_t(1) << 24)) return nav_refuse(c, who, "n must lie below 2^24");
  const float step = g->step_m > 0.0f ? g->step_m : c->cfg.voxel_size;
  const float n_steps = floorf((g->max_range_m - g->min_range_m) / step);
  if (!(n_steps < 4096.0f)) return nav_refuse(c, who, "more than 4096 samples per ray");
  if (int rc = nav_begin(c, who)) return rc;
  if (int rc = esdf_ready(c, who)) return rc;
  if (int rc = quiesce(c)) return rc;
  if (n == 0) return KS_OK;
  // the sizing rule: planes, counters, and one slab of the ball bound per workgroup in flight
  const uint32_t nt = c->esdf_tiles;
  const uint64_t side = 2 * (uint64_t)std::ceil((double)g->max_range_m / (double)c->cfg.voxel_size) + 3;
  const uint64_t ball_bits = side * side * side;
  const uint64_t slab_words = ((ball_bits + 31) / 32 + 63) / 64 * 64;   // (256-byte steps)
  const uint64_t fixed = (uint64_t)nt * kVgTileWords * 8 + sizeof(VgCounters), slab_bytes = slab_words * 4;
  if (g->max_workspace_bytes < fixed + slab_bytes) {
    if (stats) stats->workspace_bytes = fixed + slab_bytes;
    c->err = std::string(who) + ": one view in flight needs " + std::to_string(fixed + slab_bytes) + " bytes of work space, above max_workspace_bytes";
    return KS_ERR_UNSUPPORTED;
  }
  const uint64_t groups = std::min<uint64_t>(std::min<uint64_t>(n, c->vg_groups), (g->max_workspace_bytes - fixed) / slab_bytes);
  if (stats) stats->workspace_bytes = fixed + groups * slab_bytes;
  int rc;
  if ((rc = c->vg_planes.reserve(c, (size_t)nt * kVgTileWords, ((size_t)nt + nt / 2 + 64) * kVgTileWords)) || (rc = c->vg_counters.reserve(c, 1, 1)) ||
      (rc = c->vg_slabs.reserve(c, (size_t)(groups * slab_words), (size_t)(groups * slab_words))))
    return rc;
  hipStream_t st = c->stream;
  if (staged) {   // (the staging is idle: every earlier call waited for its read-back)
    if ((rc = c->vg_poses.reserve(c, 7 * n, 7 * n)) || (rc = c->vg_records.reserve(c, n, n))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->vg_poses, poses, 7 * n * sizeof(float), hipMemcpyHostToDevice, st));
    poses = c->vg_poses.get();
    d_out = c->vg_records.get();
  }
  VgParams V{};
  V.cx = g->K[2];
  V.cy = g->K[3];
  V.constant_x = (float)(1.0 / (double)g->K[0]);   // as ks_render_view
  V.constant_y = (float)(1.0 / (double)g->K[1]);
  V.width = (int)g->width;
  V.height = (int)g->height;
  V.voxel_size_inv = c->voxel_size_inv;
  V.min_range = g->min_range_m;
  V.step = step;
  V.stop_distance = g->stop_distance_m;
  V.n_samples = (uint32_t)n_steps + 1u;
  V.label = g->label;
  V.n_tiles = nt;
  V.n_views = (uint32_t)n;
  V.lds_bits = c->vg_lds_bits;
  V.ball_bits = ball_bits;
  V.slab_words = slab_words;
  HIPCHK(c, hipMemsetAsync(c->vg_counters, 0, sizeof(VgCounters), st));
  if (nt)
    hipLaunchKernelGGL(k_vg_planes, dim3(nt * 2), dim3(256), 0, st, (const EsdfRecord*)c->esdf_store.get(), V.stop_distance, V.label, c->vg_planes.get());
  hipLaunchKernelGGL(k_vg_walk, dim3((uint32_t)groups), dim3(kVgThreads), 0, st, c->table, V, poses, (const unsigned long long*)c->vg_planes.get(),
                     c->vg_slabs.get(), d_out, c->vg_counters.get());
  HIPCHK(c, hipGetLastError());
  *launched = true;
  return KS_OK;
}

// waits for the stream and reads the counters
static int view_gain_stats(ks_ctx* c, ks_view_gain_stats* stats) {
  VgCounters k{};
  HIPCHK(c, hipMemcpyAsync(&k, c->vg_counters, sizeof(k), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  stats->views_valid = k.views_valid;
  stats->views_invalid = k.views_invalid;
  stats->unknown_voxels = k.unknown;
  stats->free_voxels = k.free_;
  stats->surface_voxels = k.surface;
  stats->label_voxels = k.label;
  stats->rays_hit = k.hit;
  stats->rays_open = k.open;
  stats->samples = k.samples;
  stats->views_in_lds = k.views_in_lds;
  return KS_OK;
}

int ks_view_gain_device(ks_ctx* c, const float* d_T, size_t n, const ks_view_gain_config* g, ks_view_gain_record* d_out, ks_view_gain_stats* stats) {
  if (!c || !g) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  bool launched = false;
  if (int rc = view_gain_enqueue(c, "ks_view_gain_device", d_T, false, n, g, d_out, stats, &launched)) return rc;
  return stats && launched ? view_gain_stats(c, stats) : KS_OK;
}

int ks_view_gain(ks_ctx* c, const float* T, size_t n, const ks_view_gain_config* g, ks_view_gain_record* out, ks_view_gain_stats* stats) {
  if (!c || !g) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  bool launched = false;
  if (int rc = view_gain_enqueue(c, "ks_view_gain", T, true, n, g, out, stats, &launched)) return rc;
  hipStream_t st = c->stream;
  if (!launched) return KS_OK;
  HIPCHK(c, hipMemcpyAsync(out, c->vg_records, n * sizeof(ks_view_gain_record), hipMemcpyDeviceToHost, st));
  if (stats) return view_gain_stats(c, stats);
  HIPCHK(c, hipStreamSynchronize(st));
  return KS_OK;
}

// ---- path shortening over the stored ESDF ("Path shortening"; ks_k_path.h) ----------------------
int ks_path_shorten_default_config(ks_path_shorten_config* p) {
  if (!p) return KS_ERR_INVALID_ARG;
  std::memset(p, 0, sizeof(*p));
  p->radius_m = 0.3f;
  p->min_step_m = 0.0f;
  p->unknown_is_free = 0;
  p->max_samples = 4096;
  p->lookahead = 64;
  return KS_OK;
}

// the checks of both calls and the kernel's parameters but for its pointers; then the frames in flight are completed and the
// eight counters cleared
static int path_shorten_begin(ks_ctx* c, const char* who, const float* in, const uint32_t* n_in, size_t n, uint32_t max_waypoints,
                              const ks_path_shorten_config* p, bool any_output, PathShorten* W) {
  if (!p) return esdf_read_refuse(c, who, "the configuration is NULL");
  if (max_waypoints < 1 || max_waypoints > 65536) return esdf_read_refuse(c, who, "max_waypoints must lie in 1..65536");
  if (p->lookahead < 1 || p->lookahead > 4096) return esdf_read_refuse(c, who, "lookahead must lie in 1..4096");
  const ks_esdf_sweep_config s{p->radius_m, p->min_step_m, p->unknown_is_free, p->max_samples};
  EsdfSweep rule{};
  if (int rc = esdf_sweep_check(c, who, n, &s, &rule)) return rc;
  if (n && (!in || !n_in)) return esdf_read_refuse(c, who, "waypoints_in or n_waypoints_in is NULL");
  if (n && !any_output) return esdf_read_refuse(c, who, "all five outputs are NULL");
  if (int rc = esdf_read_begin(c, who)) return rc;
  W->n = n;
  W->max_waypoints = max_waypoints;
  W->lookahead = p->lookahead;
  W->radius = rule.radius;
  W->min_step = rule.min_step;
  W->max_length = rule.max_length;
  W->unknown_is_free = rule.unknown_is_free;
  W->max_samples = rule.max_samples;
  W->counters = c->esdf_read_counters;
  return KS_OK;
}
// k_path_shorten over W.n paths at DEVICE addresses: a wavefront per path, the grid bounded
static void path_shorten_launch(ks_ctx* c, const PathShorten& W) {
  const uint32_t blocks = (uint32_t)std::min<size_t>((W.n + 3) / 4, c->ps_blocks);
  hipLaunchKernelGGL(k_path_shorten, dim3(blocks), dim3(256), 0, c->stream, c->table, esdf_read_view(c), W);
}
static int path_shorten_stats(ks_ctx* c, ks_path_shorten_stats* stats) {
  uint64_t v[8];
  if (int rc = esdf_read_counts(c, v, 8)) return rc;
  stats->paths_ok = v[0];
  stats->paths_unverified = v[1];
  stats->paths_invalid = v[2];
  stats->waypoints_in = v[3];
  stats->waypoints_out = v[4];
  stats->segments_unverified = v[5];
  stats->sweeps = v[6];
  stats->samples = v[7];
  return KS_OK;
}

int ks_path_shorten_device(ks_ctx* c, const float* d_in, const uint32_t* d_n_in, size_t n, uint32_t max_waypoints, const ks_path_shorten_config* p,
                           uint8_t* d_status, uint32_t* d_n_out, float* d_out, float* d_length, float* d_min_clearance, ks_path_shorten_stats* stats) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  PathShorten W{};
  if (int rc = path_shorten_begin(c, "ks_path_shorten_device", d_in, d_n_in, n, max_waypoints, p,
                                  d_status || d_n_out || d_out || d_length || d_min_clearance, &W))
    return rc;
  if (n == 0) return KS_OK;
  W.in = d_in;
  W.n_in = d_n_in;
  W.status = d_status;
  W.n_out = d_n_out;
  W.out = d_out;
  W.length = d_length;
  W.min_clearance = d_min_clearance;
  path_shorten_launch(c, W);
  HIPCHK(c, hipGetLastError());
  return stats ? path_shorten_stats(c, stats) : KS_OK;
}

int ks_path_shorten(ks_ctx* c, const float* in, const uint32_t* n_in, size_t n, uint32_t max_waypoints, const ks_path_shorten_config* p, uint8_t* status,
                    uint32_t* n_out, float* out, float* length, float* min_clearance, ks_path_shorten_stats* stats) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  PathShorten W{};
  if (int rc = path_shorten_begin(c, "ks_path_shorten", in, n_in, n, max_waypoints, p, status || n_out || out || length || min_clearance, &W)) return rc;
  if (n == 0) return KS_OK;
  // a chunk's waypoints stay within 64 MiB; only the rows a path has written reach the caller's array.  out == in: in place on the
  // device as well
  const size_t row = (size_t)max_waypoints * 3;
  const size_t m_max = std::min(n, std::min(c->ps_chunk, std::max<size_t>(1, (size_t(64) << 20) / (row * sizeof(float)))));
  const bool in_place = out == in;
  int rc;
  if ((rc = c->ps_in.reserve(c, m_max * row, m_max * row)) || (rc = c->ps_u32.reserve(c, 2 * m_max, 2 * m_max)) ||
      (rc = c->ps_u8.reserve(c, m_max, m_max)) || (rc = c->ps_f.reserve(c, 2 * m_max, 2 * m_max)) ||
      (out && !in_place && (rc = c->ps_out.reserve(c, m_max * row, m_max * row))))
    return rc;
  W.in = c->ps_in.get();
  W.n_in = c->ps_u32.get();
  W.status = status ? c->ps_u8.get() : nullptr;
  W.n_out = n_out || out ? c->ps_u32.get() + m_max : nullptr;
  W.out = out ? (in_place ? c->ps_in.get() : c->ps_out.get()) : nullptr;
  W.length = length ? c->ps_f.get() : nullptr;
  W.min_clearance = min_clearance ? c->ps_f.get() + m_max : nullptr;
  std::vector<uint32_t> nw(W.n_out ? m_max : 0);
  std::vector<float> wp(out ? m_max * row : 0);
  hipStream_t st = c->stream;
  for (size_t off = 0; off < n; off += m_max) {
    const size_t m = std::min(m_max, n - off);
    HIPCHK(c, hipMemcpyAsync(c->ps_in, in + off * row, m * row * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->ps_u32, n_in + off, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    W.n = m;
    path_shorten_launch(c, W);
    if (status) HIPCHK(c, hipMemcpyAsync(status + off, W.status, m, hipMemcpyDeviceToHost, st));
    if (W.n_out) HIPCHK(c, hipMemcpyAsync(nw.data(), W.n_out, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (out) HIPCHK(c, hipMemcpyAsync(wp.data(), W.out, m * row * sizeof(float), hipMemcpyDeviceToHost, st));
    if (length) HIPCHK(c, hipMemcpyAsync(length + off, W.length, m * sizeof(float), hipMemcpyDeviceToHost, st));
    if (min_clearance) HIPCHK(c, hipMemcpyAsync(min_clearance + off, W.min_clearance, m * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));   // (the staging is reused by the next chunk)
    for (size_t i = 0; i < m; ++i) {
      if (n_out) n_out[off + i] = nw[i];
      if (out && nw[i]) std::memcpy(out + (off + i) * row, wp.data() + i * row, (size_t)nw[i] * 3 * sizeof(float));
    }
  }
  HIPCHK(c, hipGetLastError());
  return stats ? path_shorten_stats(c, stats) : KS_OK;
}

// ---- voxel-level host sync -------------------------------------------------------------------------------
// Device-side address of a host allocation the GPU can write (hipHostMalloc'ed: ks_host_alloc), else nullptr.
static void* device_view_of_pinned(void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return a.type == hipMemoryTypeHost ? a.devicePointer : nullptr;
}

static int updated_voxels_impl(ks_ctx* c, void* out, size_t cap, size_t* n, bool count_only, ks_voxel_run* runs, size_t cap_runs,
                               size_t* n_runs) {
  if (!c || !n) return KS_ERR_INVALID_ARG;
  *n = 0;
  if (n_runs) *n_runs = 0;
  if (int rc = quiesce(c)) return rc;
  const uint32_t nt = c->tiles_initialised;
  if (nt == 0) return KS_OK;
  int rc;
  if ((rc = ensure_exchange(c, (size_t)nt + 8))) return rc;
  uint32_t* d_cnt = c->d_xchg_u32;          // [0] listed tiles, [1] dirty voxels
  uint32_t* d_list = c->d_xchg_u32 + 8;
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemsetAsync(d_cnt, 0, 8 * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_list_updated_tiles, dim3((nt + 255) / 256), dim3(256), 0, st, c->pool, nt, d_list, d_cnt);
  uint32_t h_cnt[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(h_cnt, d_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const uint32_t n_list = h_cnt[0];
  if (n_list == 0) return KS_OK;
  if (n_runs) *n_runs = n_list;
  hipLaunchKernelGGL(k_export_dirty, dim3(n_list), dim3(512), 0, st, c->table, c->pool, (const uint32_t*)d_list,
                     (const uint32_t*)c->d_label_lut, c->vps_shift, 1, d_cnt, (uint8_t*)nullptr, (uint32_t*)nullptr);
  HIPCHK(c, hipMemcpyAsync(h_cnt, d_cnt, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  *n = h_cnt[1];
  if (count_only || h_cnt[1] == 0) return KS_OK;
  if ((size_t)h_cnt[1] > cap) {
    c->err = "ks_download_updated_voxels: output buffer too small (call ks_count_updated_voxels first)";
    return KS_ERR_INVALID_ARG;
  }
  if (runs && (size_t)n_list > cap_runs) {
    c->err = "ks_download_updated_voxels: run buffer too small";
    return KS_ERR_INVALID_ARG;
  }
  // pinned host targets (ks_host_alloc) are written by the kernel itself: no staging copy
  uint8_t* rec_direct = (uint8_t*)device_view_of_pinned(out);
  uint32_t* run_direct = runs ? (uint32_t*)device_view_of_pinned(runs) : nullptr;
  const size_t bytes = (size_t)h_cnt[1] * kVoxRecBytes;
  const size_t run_bytes = (size_t)n_list * sizeof(ks_voxel_run);
  const size_t need = (rec_direct ? 0 : bytes + bytes / 4) + (run_direct ? 0 : 2 * run_bytes) + 64;
  if ((!rec_direct || (runs && !run_direct)) && (rc = c->d_vox_out.reserve(c, need, need))) return rc;
  uint8_t* d_rec = rec_direct ? rec_direct : c->d_vox_out;
  uint32_t* d_runs = run_direct ? run_direct : (uint32_t*)(c->d_vox_out.get() + (rec_direct ? 0 : ((bytes + 15) & ~(size_t)15)));
  HIPCHK(c, hipMemsetAsync(d_cnt + 1, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_export_dirty, dim3(n_list), dim3(512), 0, st, c->table, c->pool, (const uint32_t*)d_list,
                     (const uint32_t*)c->d_label_lut, c->vps_shift, 0, d_cnt, d_rec, runs ? d_runs : (uint32_t*)nullptr);
  if (!rec_direct) HIPCHK(c, hipMemcpyAsync(out, c->d_vox_out, bytes, hipMemcpyDeviceToHost, st));
  if (runs && !run_direct) HIPCHK(c, hipMemcpyAsync(runs, d_runs, run_bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

int ks_count_updated_voxels(ks_ctx* c, size_t* n, size_t* n_runs) {
  return updated_voxels_impl(c, nullptr, 0, n, true, nullptr, 0, n_runs);
}
int ks_download_updated_voxels(ks_ctx* c, void* out, size_t cap, size_t* n, ks_voxel_run* runs, size_t cap_runs, size_t* n_runs) {
  if (!out && cap) return KS_ERR_INVALID_ARG;
  static_assert(sizeof(ks_voxel_run) == 20, "run record layout");
  return updated_voxels_impl(c, out, cap, n, false, runs, cap_runs, n_runs);
}

void* ks_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, std::max<size_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}

void ks_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int ks_debug_radix_sort_range(ks_ctx* c, void* keys, uint32_t* vals, size_t n, int key_bits, unsigned begin_bit, unsigned end_bit) {
  if (!c || (n && !keys) || (key_bits != 32 && key_bits != 64)) return KS_ERR_INVALID_ARG;
  if (n == 0) return KS_OK;
  const size_t kb = key_bits / 8;
  DevBuf<uint8_t> ka, kbuf;
  DevBuf<uint32_t> va, vb;
  int rc;
  if ((rc = ka.alloc(c, n * kb)) || (rc = kbuf.alloc(c, n * kb))) return rc;
  HIPCHK(c, hipMemcpy(ka, keys, n * kb, hipMemcpyHostToDevice));
  if (vals) {
    if ((rc = va.alloc(c, n)) || (rc = vb.alloc(c, n))) return rc;
    HIPCHK(c, hipMemcpy(va, vals, n * 4, hipMemcpyHostToDevice));
  }
  void* kres = nullptr;
  uint32_t* vres = nullptr;
  if (key_bits == 32) {
    uint32_t* r = nullptr;
    rc = vals ? sort_pairs(c, (uint32_t*)ka.get(), (uint32_t*)kbuf.get(), va.get(), vb.get(), n, end_bit, &r, &vres, begin_bit)
              : sort_keys(c, (uint32_t*)ka.get(), (uint32_t*)kbuf.get(), n, end_bit, &r, begin_bit);
    kres = r;
  } else {
    uint64_t* r = nullptr;
    rc = vals ? sort_pairs(c, (uint64_t*)ka.get(), (uint64_t*)kbuf.get(), va.get(), vb.get(), n, end_bit, &r, &vres, begin_bit)
              : sort_keys(c, (uint64_t*)ka.get(), (uint64_t*)kbuf.get(), n, end_bit, &r, begin_bit);
    kres = r;
  }
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(keys, kres, n * kb, hipMemcpyDeviceToHost));
  if (vals) HIPCHK(c, hipMemcpy(vals, vres, n * 4, hipMemcpyDeviceToHost));
  return KS_OK;
}

int ks_debug_radix_sort(ks_ctx* c, void* keys, uint32_t* vals, size_t n, int key_bits, unsigned end_bit) {
  return ks_debug_radix_sort_range(c, keys, vals, n, key_bits, 0u, end_bit);
}

int ks_debug_radix_sort_batch(ks_ctx* c, uint64_t* keys, uint32_t* vals, const uint64_t* counts, int nb, size_t cap, unsigned begin_bit,
                              unsigned end_bit) {
  if (!c || !keys || !vals || !counts || nb < 1 || nb > ksrs::kRsBatch || cap == 0 || cap > 0xffffffffull || begin_bit >= end_bit || end_bit > 64)
    return KS_ERR_INVALID_ARG;
  const int passes = (int)((end_bit - begin_bit + 7) / 8);
  const size_t ws_words = ksrs::ws_words_dev(cap, passes);
  DevBuf<uint64_t> ka[ksrs::kRsBatch], kb[ksrs::kRsBatch];
  DevBuf<uint32_t> va[ksrs::kRsBatch], vb[ksrs::kRsBatch], ws[ksrs::kRsBatch];
  DevBuf<unsigned long long> d_counts;
  int rc;
  if ((rc = d_counts.alloc(c, (size_t)nb))) return rc;
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counts are copied as they are");
  HIPCHK(c, hipMemcpy(d_counts, counts, (size_t)nb * sizeof(uint64_t), hipMemcpyHostToDevice));
  ksrs::DevBatch<uint64_t> B{};
  for (int y = 0; y < nb; ++y) {
    if ((rc = ka[y].alloc(c, cap)) || (rc = kb[y].alloc(c, cap)) || (rc = va[y].alloc(c, cap)) || (rc = vb[y].alloc(c, cap)) || (rc = ws[y].alloc(c, ws_words)))
      return rc;
    HIPCHK(c, hipMemcpy(ka[y], keys + (size_t)y * cap, cap * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(va[y], vals + (size_t)y * cap, cap * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(kb[y], 0xA5, cap * sizeof(uint64_t), c->stream));
    HIPCHK(c, hipMemsetAsync(vb[y], 0xA5, cap * sizeof(uint32_t), c->stream));
    B.keys_a[y] = ka[y];
    B.keys_b[y] = kb[y];
    B.vals_a[y] = va[y];
    B.vals_b[y] = vb[y];
    B.n_dev[y] = d_counts.get() + y;
    B.ws[y] = ws[y];
  }
  const hipError_t e = ksrs::sort_dev_batch<uint64_t>(B, nb, ws_words, cap, begin_bit, end_bit, c->stream);
  if (e == hipErrorInvalidValue) return KS_ERR_INVALID_ARG;   // (what the sort refuses: it has launched nothing)
  HIPCHK(c, e);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const bool in_b = (passes & 1) != 0;
  for (int y = 0; y < nb; ++y) {
    HIPCHK(c, hipMemcpy(keys + (size_t)y * cap, in_b ? kb[y].get() : ka[y].get(), cap * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(vals + (size_t)y * cap, in_b ? vb[y].get() : va[y].get(), cap * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  return KS_OK;
}

int ks_get_tile_keys(ks_ctx* c, uint64_t* out, size_t cap, size_t* n) {
  if (!c || !n) return KS_ERR_INVALID_ARG;
  if (int rc = quiesce(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n = c->tiles_initialised;
  const size_t m = std::min<size_t>(cap, *n);
  if (out && m) HIPCHK(c, hipMemcpy(out, c->table.slot_keys, m * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return KS_OK;
}

int ks_export_tiles_device(ks_ctx* c, const uint32_t* slots, size_t n, void* d_payload) {
  if (!c || (n && (!slots || !d_payload))) return KS_ERR_INVALID_ARG;
  if (n == 0) return KS_OK;
  if (int rc = quiesce(c)) return rc;
  for (size_t i = 0; i < n; ++i)
    if (slots[i] >= c->tiles_initialised) return KS_ERR_INVALID_ARG;
  if (int rc = ensure_exchange(c, n)) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_xchg_u32, slots, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_export_tiles, dim3((uint32_t)n), dim3(512), 0, c->stream, c->pool, c->d_xchg_u32, (uint4*)d_payload);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KS_OK;
}

int ks_merge_tiles_device(ks_ctx* c, const uint64_t* keys, size_t n, const void* d_payload) {
  if (!c || (n && (!keys || !d_payload))) return KS_ERR_INVALID_ARG;
  if (n == 0) return KS_OK;
  if (c->fatal) return KS_ERR_INVALID_ARG;
  // group the incoming tiles by key, keeping the caller's order inside a group
  std::vector<uint32_t> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  std::vector<uint64_t> ukeys;
  std::vector<uint32_t> offs;
  for (size_t i = 0; i < n; ++i) {
    if (i == 0 || keys[order[i]] != keys[order[i - 1]]) {
      ukeys.push_back(keys[order[i]]);
      offs.push_back((uint32_t)i);
    }
  }
  offs.push_back((uint32_t)n);
  const size_t nu = ukeys.size();
  int rc;
  if ((rc = quiesce(c))) return rc;
  if ((rc = ensure_exchange(c, n + 1))) return rc;
  uint32_t* d_offs = c->d_xchg_u32;
  uint32_t* d_idx = c->d_xchg_u32 + (nu + 1);
  HIPCHK(c, hipMemcpyAsync(c->d_xchg_u64, ukeys.data(), nu * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_offs, offs.data(), (nu + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_idx, order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  // allocate tiles this rank has not seen yet
  if ((rc = insert_tiles(c, c->d_xchg_u64, nu))) return rc;
  switch (c->cfg.color_mode) {
    case KS_COLOR_MODE_COLOR:
      hipLaunchKernelGGL(k_merge_tiles<KS_COLOR_MODE_COLOR>, dim3((uint32_t)nu), dim3(512), 0, c->stream, c->table, c->pool,
                         c->d_xchg_u64, d_offs, d_idx, (const uint4*)d_payload, c->cfg.max_weight, c->d_label_lut);
      break;
    case KS_COLOR_MODE_SEMANTIC:
      hipLaunchKernelGGL(k_merge_tiles<KS_COLOR_MODE_SEMANTIC>, dim3((uint32_t)nu), dim3(512), 0, c->stream, c->table,
                         c->pool, c->d_xchg_u64, d_offs, d_idx, (const uint4*)d_payload, c->cfg.max_weight, c->d_label_lut);
      break;
    default:
      hipLaunchKernelGGL(k_merge_tiles<KS_COLOR_MODE_SEMANTIC_PROBABILITY>, dim3((uint32_t)nu), dim3(512), 0, c->stream,
                         c->table, c->pool, c->d_xchg_u64, d_offs, d_idx, (const uint4*)d_payload, c->cfg.max_weight,
                         c->d_label_lut);
      break;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return KS_OK;
}

int ks_reset_tiles(ks_ctx* c, const uint32_t* slots, size_t n) {
  if (!c || (n && !slots)) return KS_ERR_INVALID_ARG;
  if (n == 0) return KS_OK;
  if (int rc = quiesce(c)) return rc;
  for (size_t i = 0; i < n; ++i)
    if (slots[i] >= c->tiles_initialised) return KS_ERR_INVALID_ARG;
  if (int rc = ensure_exchange(c, n)) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_xchg_u32, slots, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_reset_tiles, dim3((uint32_t)n), dim3(512), 0, c->stream, c->pool, c->d_xchg_u32);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KS_OK;
}

// ---- ks_reduce: the frame-sharded path's one exchange step, through RCCL ------------------
// librccl is loaded on first use (the library itself has no link-time dependency on it); the communicator
// is the caller's.  KS_RCCL_LIB overrides the path.
namespace {
struct RcclApi {
  void* h = nullptr;
  decltype(&ncclAllGather) all_gather = nullptr;
  decltype(&ncclSend) send = nullptr;
  decltype(&ncclRecv) recv = nullptr;
  decltype(&ncclGroupStart) group_start = nullptr;
  decltype(&ncclGroupEnd) group_end = nullptr;
  decltype(&ncclGetErrorString) err_string = nullptr;
  bool load(std::string* why) {
    if (h) return true;
    const char* env = getenv("KS_RCCL_LIB");
    const char* names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* nm : names) {
      if (!nm) continue;
      h = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
      if (h) break;
    }
    if (!h) { *why = "librccl not found (set KS_RCCL_LIB)"; return false; }
    all_gather = (decltype(all_gather))dlsym(h, "ncclAllGather");
    send = (decltype(send))dlsym(h, "ncclSend");
    recv = (decltype(recv))dlsym(h, "ncclRecv");
    group_start = (decltype(group_start))dlsym(h, "ncclGroupStart");
    group_end = (decltype(group_end))dlsym(h, "ncclGroupEnd");
    err_string = (decltype(err_string))dlsym(h, "ncclGetErrorString");
    if (!all_gather || !send || !recv || !group_start || !group_end) { *why = "librccl lacks a required symbol"; h = nullptr; return false; }
    return true;
  }
};
RcclApi g_rccl;

inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
}  // namespace

#define NCCLCHK(ctx, expr)                                                                                    \
  do {                                                                                                        \
    ncclResult_t r_ = (expr);                                                                                 \
    if (r_ != ncclSuccess) {                                                                                  \
      (ctx)->err = std::string(#expr) + ": " + (g_rccl.err_string ? g_rccl.err_string(r_) : "rccl error");    \
      return KS_ERR_HIP;                                                                                      \
    }                                                                                                         \
  } while (0)

int ks_tile_owner(uint64_t tile_key, int world) { return world > 0 ? (int)(splitmix64(tile_key) % (uint64_t)world) : 0; }

// grow-only scratch of ks_reduce (no allocation in the steady state)
static int ensure_reduce_scratch(ks_ctx* c, size_t n_send, size_t n_recv, int world) {
  int rc;
  // [world] own | [world x world] all | [world] offsets | [world] cursors
  if ((rc = c->d_rx_counts.reserve(c, (size_t)(world + 3) * world, (size_t)(world + 3) * world))) return rc;
  if (n_send > c->cap_tx) {
    const size_t cap = std::max<size_t>(n_send + n_send / 2, 64);
    c->cap_tx = 0;
    if ((rc = c->d_tx_keys.alloc(c, cap))) return rc;
    if ((rc = c->d_tx_slots.alloc(c, cap))) return rc;
    if ((rc = c->d_tx_payload.alloc(c, cap * (size_t)KS_TILE_BYTES))) return rc;
    c->cap_tx = cap;
  }
  if (n_recv > c->cap_rx) {
    const size_t cap = std::max<size_t>(n_recv + n_recv / 2, 64);
    c->cap_rx = 0;
    if ((rc = c->d_rx_keys.alloc(c, cap))) return rc;
    if ((rc = c->d_rx_payload.alloc(c, cap * (size_t)KS_TILE_BYTES))) return rc;
    c->cap_rx = cap;
  }
  return KS_OK;
}

// COLLECTIVE: every rank of the communicator must call it (a rank that returns early on a local error leaves its
// peers waiting in the exchange, as with any RCCL collective).
int ks_reduce(ks_ctx* c, void* rccl_comm, int rank, int world, ks_reduce_stats* stats) {
  if (!c || world < 1 || rank < 0 || rank >= world || (world > 1 && !rccl_comm)) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (c->fatal) return KS_ERR_INVALID_ARG;
  int rc;
  if ((rc = quiesce(c))) return rc;
  const uint32_t nt = c->tiles_initialised;
  if (stats) stats->tiles_local = nt;
  hipStream_t st = c->stream;
  if (world == 1) {  // everything is owned here: nothing travels
    if (nt) HIPCHK(c, hipMemsetAsync(c->pool.dirty, 0, nt, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return KS_OK;
  }
  std::string why;
  if (!g_rccl.load(&why)) {
    c->err = why;
    return KS_ERR_UNSUPPORTED;
  }
  ncclComm_t comm = (ncclComm_t)rccl_comm;
  if ((rc = ensure_reduce_scratch(c, 0, 0, world))) return rc;
  // 1) what goes where, counted on the device: tiles touched since the last reduce that another rank owns;
  //    every rank learns every rank's counts (world x world int32) in the same breath
  int32_t* d_own = c->d_rx_counts;
  int32_t* d_all = d_own + world;
  uint32_t* d_offs = (uint32_t*)(d_all + (size_t)world * world);
  uint32_t* d_cursor = d_offs + world;
  HIPCHK(c, hipMemsetAsync(d_own, 0, (size_t)(world + 3) * world * sizeof(int32_t), st));
  const uint32_t nb = (nt + 255) / 256;
  if (nt)
    hipLaunchKernelGGL(k_dirty_by_owner, dim3(nb), dim3(256), 0, st, c->pool, (const uint64_t*)c->table.slot_keys, nt, (uint32_t)rank,
                       (uint32_t)world, 0, d_own, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint64_t*)nullptr);
  NCCLCHK(c, g_rccl.all_gather(d_own, d_all, (size_t)world, ncclInt32, comm, st));
  std::vector<int32_t> all_counts((size_t)world * world);
  HIPCHK(c, hipMemcpyAsync(all_counts.data(), d_all, all_counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  std::vector<size_t> send_counts(world), recv_counts(world), recv_off(world + 1, 0), send_off(world + 1, 0);
  for (int p = 0; p < world; ++p) {
    send_counts[p] = (size_t)all_counts[(size_t)rank * world + p];
    recv_counts[p] = (size_t)all_counts[(size_t)p * world + rank];
    send_off[p + 1] = send_off[p] + send_counts[p];
    recv_off[p + 1] = recv_off[p] + recv_counts[p];
  }
  const size_t n_send = send_off[world], n_recv = recv_off[world];
  if ((rc = ensure_reduce_scratch(c, n_send, n_recv, world))) return rc;
  // 2) the send list (slots + keys grouped by owner) and the raw tile records, all on the device
  if (n_send) {
    std::vector<uint32_t> offs32(world);
    for (int p = 0; p < world; ++p) offs32[p] = (uint32_t)send_off[p];
    HIPCHK(c, hipMemcpyAsync(d_offs, offs32.data(), world * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_dirty_by_owner, dim3(nb), dim3(256), 0, st, c->pool, (const uint64_t*)c->table.slot_keys, nt, (uint32_t)rank,
                       (uint32_t)world, 1, d_own, (const uint32_t*)d_offs, d_cursor, c->d_tx_slots, c->d_tx_keys);
    hipLaunchKernelGGL(k_export_tiles, dim3((uint32_t)n_send), dim3(512), 0, st, c->pool, (const uint32_t*)c->d_tx_slots,
                       (uint4*)c->d_tx_payload.get());
    HIPCHK(c, hipStreamSynchronize(st));  // (offs32 is a stack-side buffer)
  }
  // 3) keys and raw tile records: one grouped exchange — on a fully connected xGMI node a rank talks to all its
  //    peers at once (a ring all-reduce would be per-link bound and move every tile through every rank)
  NCCLCHK(c, g_rccl.group_start());
  for (int peer = 0; peer < world; ++peer) {
    if (peer == rank) continue;
    if (send_counts[peer]) {
      NCCLCHK(c, g_rccl.send(c->d_tx_keys + send_off[peer], send_counts[peer], ncclUint64, peer, comm, st));
      NCCLCHK(c, g_rccl.send(c->d_tx_payload + send_off[peer] * (size_t)KS_TILE_BYTES, send_counts[peer] * (size_t)KS_TILE_BYTES,
                             ncclUint8, peer, comm, st));
    }
    if (recv_counts[peer]) {
      NCCLCHK(c, g_rccl.recv(c->d_rx_keys + recv_off[peer], recv_counts[peer], ncclUint64, peer, comm, st));
      NCCLCHK(c, g_rccl.recv(c->d_rx_payload + recv_off[peer] * (size_t)KS_TILE_BYTES, recv_counts[peer] * (size_t)KS_TILE_BYTES,
                             ncclUint8, peer, comm, st));
    }
  }
  NCCLCHK(c, g_rccl.group_end());
  std::vector<uint64_t> k_host(n_recv);
  if (n_recv) HIPCHK(c, hipMemcpyAsync(k_host.data(), c->d_rx_keys, n_recv * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  // 4) the owner folds what it received into its map, tiles of one key in ascending source-rank order
  //    (the receive buffer is ordered by source rank), in one launch
  if (n_recv && (rc = ks_merge_tiles_device(c, k_host.data(), n_recv, c->d_rx_payload))) return rc;
  // 5) what was sent starts over as an empty delta here: a later reduce cannot count it twice
  if (n_send) hipLaunchKernelGGL(k_reset_tiles, dim3((uint32_t)n_send), dim3(512), 0, st, c->pool, (const uint32_t*)c->d_tx_slots);
  HIPCHK(c, hipMemsetAsync(c->pool.dirty, 0, c->tiles_initialised, st));  // owned tiles: authoritative here, nothing pending
  HIPCHK(c, hipStreamSynchronize(st));
  if (stats) {
    stats->tiles_sent = n_send;
    stats->tiles_received = n_recv;
    stats->bytes_sent = n_send * (uint64_t)(KS_TILE_BYTES + 8);
  }
  return KS_OK;
}

// Owner: one frame's records (of the tiles this rank owns, in integration order) into the map.  `merged`: the frame's two
// tables come with them (ks_k_shard_merged.h).
struct ShardTables {
  const float2* btab;
  uint32_t n_bundles;
  const float* mixed;
  uint32_t n_mixed;
};
static int shard_apply_segment(ks_ctx* o, const uint64_t* d_gkey, const uint32_t* d_seq, const float* d_sdf, const float* d_uw, size_t n,
                               size_t tiles_at_most, const ShardTables* mt = nullptr) {
  if (n == 0) return KS_OK;
  if (n >= (size_t)1 << 31) { o->err = "ks_integrate_round_exact: more than 2^31 updates of one frame for one owner"; return KS_ERR_INVALID_ARG; }
  int rc;
  if (n > o->cap_sh_rx) {
    const size_t cap = std::max<size_t>(n + n / 4, 1 << 18);
    o->cap_sh_rx = 0;
    if ((rc = o->d_sh_tk.alloc(o, cap))) return rc;
    for (int b = 0; b < 2; ++b) {
      if ((rc = o->d_sh_pairs[b].alloc(o, cap))) return rc;
      if ((rc = o->d_sh_vals[b].alloc(o, cap))) return rc;
    }
    o->cap_sh_rx = cap;
  }
  if (mt && n > o->cap_shm_ops) {
    const size_t cap = std::max<size_t>(n + n / 4, 1 << 18);
    o->cap_shm_ops = 0;
    if ((rc = o->d_shm_ops.alloc(o, cap))) return rc;
    if ((rc = o->d_shm_long.alloc(o, cap / (kLongRun + 1) + 2))) return rc;   // a long run has more than kLongRun updates
    o->cap_shm_ops = cap;
  }
  hipStream_t st = o->stream;
  const uint32_t nb = (uint32_t)((n + 255) / 256);
  hipLaunchKernelGGL(k_shard_tile_keys, dim3(nb), dim3(256), 0, st, (uint32_t)n, d_gkey, o->d_sh_tk);
  // get-or-insert + initialisation of the new tiles (the pool grows if it must; the records cannot name more tiles than the rank
  // that marched the frame has ever numbered)
  if ((rc = insert_tiles(o, o->d_sh_tk, n, tiles_at_most))) return rc;
  hipLaunchKernelGGL(k_shard_import, dim3(nb), dim3(256), 0, st, (uint32_t)n, o->table, o->pool, d_gkey, d_seq, o->d_sh_pairs[0], o->d_sh_vals[0]);
  const unsigned end_bit = kShardSeqBits + 9 + bits_for(o->tiles_initialised);
  uint64_t* kres = nullptr;
  uint32_t* vres = nullptr;
  // stable: a voxel's updates stay in the order they were emitted in = the integration order
  HIPCHK(o, (ksrs::sort<uint64_t, true>(o->sort_ws, o->d_sh_pairs[0], o->d_sh_pairs[1], o->d_sh_vals[0], o->d_sh_vals[1], n, std::min(56u, end_bit), st,
                                        &kres, &vres, kShardSeqBits)));
  FrameParams F{};
  const ks_config& cfg = o->cfg;
  F.log_match = o->log_match;
  F.log_non_match = o->log_non_match;
  F.tsdf.voxel_size = cfg.voxel_size;
  F.tsdf.trunc = cfg.truncation_distance;
  F.tsdf.max_weight = cfg.max_weight;
  F.tsdf.dropoff_denominator = cfg.truncation_distance - cfg.voxel_size;
  F.tsdf.sparsity_factor = cfg.sparsity_compensation_factor;
  F.tsdf.use_dropoff = cfg.use_weight_dropoff;
  F.tsdf.use_sparsity = cfg.use_sparsity_compensation_factor;
  if (mt) {
    // the operands in run order and the long runs' heads; then short runs a lane each, long runs two wavefronts each
    uint32_t* const d_n_long = o->d_shm_long + (o->cap_shm_ops / (kLongRun + 1) + 1);
    HIPCHK(o, hipMemsetAsync(d_n_long, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_shard_stage_merged, dim3(nb), dim3(256), 0, st, (uint32_t)n, mt->n_bundles, (const uint64_t*)kres, (const uint32_t*)vres, d_sdf,
                       d_uw, mt->btab, o->d_shm_ops, o->d_shm_long, d_n_long);
    const uint32_t lb = (uint32_t)std::min<size_t>(2 * (n / (kLongRun + 1) + 1), 4096);
#define KS_LAUNCH_SHARD_MERGED(MODE)                                                                                                         \
  hipLaunchKernelGGL(k_shard_apply_merged<MODE>, dim3(nb), dim3(256), 0, st, F.tsdf, (uint32_t)n, mt->n_mixed, (const uint64_t*)kres,         \
                     (const float4*)o->d_shm_ops, mt->mixed, o->pool, (const uint32_t*)o->d_label_lut);                                      \
  hipLaunchKernelGGL(k_shard_apply_merged_long<MODE>, dim3(lb), dim3(64), 0, st, F.tsdf, (uint32_t)n, mt->n_mixed, (const uint64_t*)kres,     \
                     (const float4*)o->d_shm_ops, mt->mixed, o->pool, (const uint32_t*)o->d_label_lut, (const uint32_t*)o->d_shm_long,       \
                     (const uint32_t*)d_n_long)
    if (cfg.color_mode == KS_COLOR_MODE_SEMANTIC) {
      KS_LAUNCH_SHARD_MERGED(KS_COLOR_MODE_SEMANTIC);
    } else {
      KS_LAUNCH_SHARD_MERGED(KS_COLOR_MODE_SEMANTIC_PROBABILITY);
    }
#undef KS_LAUNCH_SHARD_MERGED
  } else if (cfg.color_mode == KS_COLOR_MODE_SEMANTIC)
    hipLaunchKernelGGL(k_shard_apply<KS_COLOR_MODE_SEMANTIC>, dim3(nb), dim3(256), 0, st, F, (uint32_t)n, (const uint64_t*)kres, (const uint32_t*)vres, d_sdf,
                       d_uw, o->pool, (const uint32_t*)o->d_label_lut);
  else
    hipLaunchKernelGGL(k_shard_apply<KS_COLOR_MODE_SEMANTIC_PROBABILITY>, dim3(nb), dim3(256), 0, st, F, (uint32_t)n, (const uint64_t*)kres,
                       (const uint32_t*)vres, d_sdf, d_uw, o->pool, (const uint32_t*)o->d_label_lut);
  HIPCHK(o, hipStreamSynchronize(st));
  HIPCHK(o, hipGetLastError());
  return KS_OK;
}

// The text goes to both contexts: the caller may ask either for it.
static int round_fail(ks_ctx* m, ks_ctx* o, int rc, const std::string& why) {
  m->err = why;
  o->err = why;
  return rc;
}

int ks_integrate_round_exact(ks_ctx* m, ks_ctx* o, void* rccl_comm, int rank, int world, uint64_t first_frame, const float T[7],
                             const float* xyz, const uint8_t* rgba, const uint8_t* labels, size_t n, int freespace, ks_round_stats* stats) {
  if (!m || !o || m == o || !T || world < 1 || world > 64 || rank < 0 || rank >= world || (world > 1 && !rccl_comm) || (n && !xyz))
    return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  // ---- what is the same on every rank (the configuration, by contract): refused before anything is exchanged ----
  if (m->cfg.method != o->cfg.method)
    return round_fail(m, o, KS_ERR_UNSUPPORTED, "ks_integrate_round_exact: marcher and owner must be created with the same method");
  const bool merged = m->cfg.method == KS_METHOD_MERGED;
  for (ks_ctx* c : {m, o}) {
    const ks_config& k = c->cfg;
    if (merged) {
      if (k.color_mode == KS_COLOR_MODE_COLOR)
        return round_fail(m, o, KS_ERR_UNSUPPORTED,
                          "ks_integrate_round_exact: color_mode = KS_COLOR_MODE_COLOR blends the voxel's colour with the bundle's by the voxel's "
                          "weight at that update, which an update record does not carry: colours from the labels only (anything else: integrate "
                          "per rank and ks_reduce)");
      if (k.pipeline_frames != 0)
        return round_fail(m, o, KS_ERR_UNSUPPORTED, "ks_integrate_round_exact: one frame at a time (pipeline_frames = 0)");
      continue;
    }
    const bool frames_independent = !c->uses_early_out || k.clear_checks_every_n_frames <= 1;
    if (k.method != KS_METHOD_FAST || k.color_mode == KS_COLOR_MODE_COLOR || k.pipeline_frames != 0 || !frames_independent ||
        k.integration_order_mode == KS_ORDER_SORTED)
      return round_fail(m, o, KS_ERR_UNSUPPORTED,
                        "ks_integrate_round_exact: `fast`, colours from the labels, one frame at a time, mixed order, clear_checks_every_n_frames = 1 "
                        "(anything else: integrate per rank and ks_reduce)");
  }
  if (world > 1) {
    std::string why;
    if (!g_rccl.load(&why)) return round_fail(m, o, KS_ERR_UNSUPPORTED, why);   // (no library, no exchange: nothing a peer could be told through)
  }
  // ---- what can differ from rank to rank: a failure here is CARRIED to the peers in the count exchange below, no rank is left
  //      waiting, every rank returns an error and nothing of the round is applied anywhere ----
  const uint64_t seen_before = m->shard_frames_seen;
  bool marcher_moved = false;   // the marcher's per-call state (the approximate sets' offsets of `fast`) has advanced
  ks_frame_stats fst{};
  auto march = [&]() -> int {
    int rc;
    if (m->fatal || o->fatal)
      return round_fail(m, o, KS_ERR_INVALID_ARG, "ks_integrate_round_exact: a context is unusable after an earlier failure (destroy it)");
    if (n >= ((size_t)1 << kShardSeqBits))
      return round_fail(m, o, KS_ERR_INVALID_ARG, "ks_integrate_round_exact: a cloud of 2^24 points or more does not fit the update record's position field");
    const uint64_t my_frame = first_frame + (uint64_t)rank;
    if (m->shard_frames_seen > my_frame) return round_fail(m, o, KS_ERR_INVALID_ARG, "ks_integrate_round_exact: rounds must come in frame order");
    m->shard_export = true;
    m->shard_world = world;
    static const uint8_t no_label = 0;
    if (merged) {
      // nothing of `merged` outlives a frame (ks_k_shard_merged.h): the frames of the other ranks are only counted
      m->shard_frames_seen = my_frame;
    } else {
      // the frames other ranks march in between advance this marcher's set offsets and frame counters like empty clouds
      // ([K:src/semantic_tsdf_integrator_fast.cpp:165-170]: the bookkeeping is per call)
      const float T0[7] = {1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (; m->shard_frames_seen < my_frame; ++m->shard_frames_seen) {
        marcher_moved = true;
        if ((rc = ks_integrate_points(m, T0, nullptr, nullptr, &no_label, 0, 0, nullptr))) return rc;
      }
    }
    std::memset(m->sh_counts, 0, sizeof(m->sh_counts));
    m->sh_exported = 0;
    m->shm_counts[0] = m->shm_counts[1] = 0;
    marcher_moved = marcher_moved || !merged;
    if ((rc = ks_integrate_points(m, T, xyz, rgba, labels ? labels : (rgba ? nullptr : &no_label), n, freespace, &fst))) return rc;
    ++m->shard_frames_seen;
    uint64_t sum = 0;
    for (int p = 0; p < world; ++p) sum += m->sh_counts[p];
    if (sum != m->sh_exported) return round_fail(m, o, KS_ERR_HIP, "ks_integrate_round_exact: the per-owner counts do not add up to the frame's updates");
    return KS_OK;
  };
  // a round that failed has to be repeated by every rank: the marcher is put back where it was, or, where its state cannot be
  // (`fast`: the sets' offsets have moved), retired
  auto undo = [&]() {
    if (marcher_moved) {
      m->fatal = true;
    } else {
      m->shard_frames_seen = seen_before;
    }
  };
  int rc = march();
  if (rc) {  // nothing leaves this rank but its error code
    std::memset(m->sh_counts, 0, sizeof(m->sh_counts));
    m->sh_exported = 0;
    m->shm_counts[0] = m->shm_counts[1] = 0;
    o->err = m->err;
  }
  // where this frame's records sit, by owner
  std::vector<size_t> send_counts(world), send_off(world + 1, 0);
  for (int p = 0; p < world; ++p) {
    send_counts[p] = m->sh_counts[p];
    send_off[p + 1] = send_off[p] + send_counts[p];
  }
  const ShardTables own_tables{m->d_shm_btab, m->shm_counts[0], m->d_shm_mixed, m->shm_counts[1]};
  uint64_t applied = 0, origin = merged ? 0 : m->sh_counts[world];
  if (world == 1) {
    if (rc) {
      undo();
      return rc;
    }
    if ((rc = shard_apply_segment(o, m->d_sh_gkey[1], m->d_sh_seq[1], m->d_sh_sdf[1], m->d_sh_uw[1], send_counts[0], m->tiles_initialised,
                                  merged ? &own_tables : nullptr)))
      return rc;
    applied = send_counts[0];
  } else {
    ncclComm_t comm = (ncclComm_t)rccl_comm;
    hipStream_t st = o->stream;
    // 1) everybody's row: [world] counts | origin-voxel flag | marcher's tile count | bundles | mixed-label bundles | error code
    const int W2 = world + 5;
    int arc;
    if ((arc = ensure_reduce_scratch(o, 0, 0, W2))) return arc;
    int32_t* d_own = o->d_rx_counts;
    int32_t* d_all = d_own + W2;
    std::vector<int32_t> own(W2);
    for (int p = 0; p < world; ++p) own[p] = (int32_t)send_counts[p];
    own[world] = (int32_t)origin;
    own[world + 1] = (int32_t)m->tiles_initialised;
    own[world + 2] = (int32_t)m->shm_counts[0];
    own[world + 3] = (int32_t)m->shm_counts[1];
    own[world + 4] = (int32_t)rc;
    HIPCHK(o, hipMemcpyAsync(d_own, own.data(), own.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    NCCLCHK(o, g_rccl.all_gather(d_own, d_all, (size_t)W2, ncclInt32, comm, st));
    std::vector<int32_t> all((size_t)W2 * world);
    HIPCHK(o, hipMemcpyAsync(all.data(), d_all, all.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(o, hipStreamSynchronize(st));
    for (int p = 0; p < world; ++p) {
      const int prc = all[(size_t)p * W2 + world + 4];
      if (!prc) continue;
      // every rank sees the same rows: all of them leave here, before the exchange
      undo();
      if (rc) return rc;   // (this rank's own failure: its code, its text)
      return round_fail(m, o, KS_ERR_PEER_FAILED,
                        "ks_integrate_round_exact: rank " + std::to_string(p) + " failed with code " + std::to_string(prc) +
                            " (its ks_last_error says why); nothing of this round was applied on any rank");
    }
    std::vector<size_t> recv_counts(world), recv_off(world + 1, 0), rb_off(world + 1, 0), rm_off(world + 1, 0);
    for (int p = 0; p < world; ++p) {
      const int32_t* row = &all[(size_t)p * W2];
      recv_counts[p] = p == rank ? 0 : (size_t)row[rank];
      recv_off[p + 1] = recv_off[p] + recv_counts[p];
      // (a peer's tables travel only with records)
      rb_off[p + 1] = rb_off[p] + (merged && recv_counts[p] ? (size_t)row[world + 2] : 0);
      rm_off[p + 1] = rm_off[p] + (merged && recv_counts[p] ? (size_t)row[world + 3] : 0);
      origin |= (uint64_t)row[world];
    }
    const size_t n_recv = recv_off[world];
    // 2) receive buffers on the owner context (its own d_sh_*[0]: an owner context never exports)
    if (n_recv > o->cap_sh) {
      const size_t cap = std::max<size_t>(n_recv + n_recv / 4, 1 << 18);
      o->cap_sh = 0;
      if ((rc = o->d_sh_gkey[0].alloc(o, cap))) return rc;
      if ((rc = o->d_sh_seq[0].alloc(o, cap))) return rc;
      if ((rc = o->d_sh_sdf[0].alloc(o, cap))) return rc;
      if ((rc = o->d_sh_uw[0].alloc(o, cap))) return rc;
      o->cap_sh = cap;
    }
    if ((rc = o->d_shm_rx_btab.reserve(o, rb_off[world], std::max<size_t>(rb_off[world] + rb_off[world] / 4, 1 << 14)))) return rc;
    if ((rc = o->d_shm_rx_mixed.reserve(o, rm_off[world] * kNumLabels, std::max<size_t>(rm_off[world] + rm_off[world] / 4, 1 << 10) * kNumLabels))) return rc;
    // 3) one grouped exchange: every rank talks to all its peers at once (xGMI is point to point)
    uint64_t bytes = 0;
    NCCLCHK(o, g_rccl.group_start());
    for (int peer = 0; peer < world; ++peer) {
      if (peer == rank) continue;
      if (send_counts[peer]) {
        NCCLCHK(o, g_rccl.send(m->d_sh_gkey[1] + send_off[peer], send_counts[peer], ncclUint64, peer, comm, st));
        NCCLCHK(o, g_rccl.send(m->d_sh_seq[1] + send_off[peer], send_counts[peer], ncclUint32, peer, comm, st));
        NCCLCHK(o, g_rccl.send(m->d_sh_sdf[1] + send_off[peer], send_counts[peer], ncclFloat32, peer, comm, st));
        NCCLCHK(o, g_rccl.send(m->d_sh_uw[1] + send_off[peer], send_counts[peer], ncclFloat32, peer, comm, st));
        bytes += send_counts[peer] * 20ull;
        if (merged && own_tables.n_bundles) {
          NCCLCHK(o, g_rccl.send(own_tables.btab, (size_t)own_tables.n_bundles * 2, ncclFloat32, peer, comm, st));
          bytes += own_tables.n_bundles * 8ull;
        }
        if (merged && own_tables.n_mixed) {
          NCCLCHK(o, g_rccl.send(own_tables.mixed, (size_t)own_tables.n_mixed * kNumLabels, ncclFloat32, peer, comm, st));
          bytes += own_tables.n_mixed * (uint64_t)(kNumLabels * sizeof(float));
        }
      }
      if (recv_counts[peer]) {
        NCCLCHK(o, g_rccl.recv(o->d_sh_gkey[0] + recv_off[peer], recv_counts[peer], ncclUint64, peer, comm, st));
        NCCLCHK(o, g_rccl.recv(o->d_sh_seq[0] + recv_off[peer], recv_counts[peer], ncclUint32, peer, comm, st));
        NCCLCHK(o, g_rccl.recv(o->d_sh_sdf[0] + recv_off[peer], recv_counts[peer], ncclFloat32, peer, comm, st));
        NCCLCHK(o, g_rccl.recv(o->d_sh_uw[0] + recv_off[peer], recv_counts[peer], ncclFloat32, peer, comm, st));
        if (rb_off[peer + 1] > rb_off[peer])
          NCCLCHK(o, g_rccl.recv(o->d_shm_rx_btab + rb_off[peer], (rb_off[peer + 1] - rb_off[peer]) * 2, ncclFloat32, peer, comm, st));
        if (rm_off[peer + 1] > rm_off[peer])
          NCCLCHK(o, g_rccl.recv(o->d_shm_rx_mixed + rm_off[peer] * kNumLabels, (rm_off[peer + 1] - rm_off[peer]) * kNumLabels, ncclFloat32, peer,
                                 comm, st));
      }
    }
    NCCLCHK(o, g_rccl.group_end());
    HIPCHK(o, hipStreamSynchronize(st));
    // 4) the frames of the round in frame order = in the order of the ranks that marched them
    for (int src = 0; src < world; ++src) {
      if (src == rank) {
        if ((rc = shard_apply_segment(o, m->d_sh_gkey[1] + send_off[rank], m->d_sh_seq[1] + send_off[rank], m->d_sh_sdf[1] + send_off[rank],
                                      m->d_sh_uw[1] + send_off[rank], send_counts[rank], m->tiles_initialised, merged ? &own_tables : nullptr)))
          return rc;
        applied += send_counts[rank];
      } else {
        const int32_t* row = &all[(size_t)src * W2];
        const ShardTables rx{o->d_shm_rx_btab + rb_off[src], (uint32_t)(rb_off[src + 1] - rb_off[src]),
                             o->d_shm_rx_mixed + rm_off[src] * kNumLabels, (uint32_t)(rm_off[src + 1] - rm_off[src])};
        if ((rc = shard_apply_segment(o, o->d_sh_gkey[0] + recv_off[src], o->d_sh_seq[0] + recv_off[src], o->d_sh_sdf[0] + recv_off[src],
                                      o->d_sh_uw[0] + recv_off[src], recv_counts[src], (size_t)row[world + 1], merged ? &rx : nullptr)))
          return rc;
        applied += recv_counts[src];
      }
    }
    if (stats) stats->bytes_sent = bytes;
  }
  if (stats) {
    stats->updates_marched = m->sh_exported;
    stats->updates_applied = applied;
    stats->origin_voxel_touched = origin ? 1 : 0;
    stats->rays_cast = fst.n_rays_cast;
  }
  return KS_OK;
}


// keep_integrator_state: only the MAP goes (tile table, pool flags); the two approximate sets, their offsets, the
// frame counters and the early-out table stay as the frames so far left them — what vxb::TsdfServer::clear() does to the
// reference's integrator, which it does not touch.  Frames in flight are completed first (their stage B has already
// entered its marks); without it a frame that was never applied is dropped with the map.
static void mesh_reset(ks_ctx* c) {
  c->mesh_valid = false;
  c->mi_valid = false;     // (the indexed view of the mesh)
  c->mesh_blocks.clear();
  c->mesh_dir.clear();
  c->mesh_changed.clear();
  c->mesh_tiles_seen = 0;
  c->esdf_valid = false;   // the stored ESDF goes with the map
  c->esdf_tiles = 0;
  c->esdf_changed.clear();
  c->esdf_removed.clear();
  c->mesh_removed.clear();
  c->obj_valid = false;    // ... and the stored objects
  c->obj_tiles = 0;
  c->obj_count = 0;
  c->nav_valid = false;    // ... and the navigation field
  c->nav_tiles = 0;
  drop_frontiers(c);       // ... and the frontiers
  c->fr_tiles = 0;
  drop_rooms(c);           // ... and the rooms
  c->rooms_tiles = 0;
}
static int clear_impl(ks_ctx* c, bool keep_integrator_state) {
  if (keep_integrator_state) {
    if (int rc = quiesce(c)) return rc;
    c->owed = ks_frame_stats{};
  }
  for (auto& S : c->slot) S.pending = false;  // a frame that was never applied is dropped with the map
  c->batch_slots.clear();
  c->owed = ks_frame_stats{};
  if (c->stream_tail != c->stream) HIPCHK(c, hipStreamSynchronize(c->stream_tail));
  HIPCHK(c, hipStreamSynchronize(c->stream_long));  // (long runs of the last frame: deferred join)
  c->pending_join = nullptr;
  if (int rc = sync_march(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemset(c->table.ent, 0xff, ((size_t)c->table.mask + 1) * sizeof(TileEntry)));
  HIPCHK(c, hipMemset(c->pool.updated, 0, c->cfg.max_tiles));
  HIPCHK(c, hipMemset(c->pool.dirty, 0, c->cfg.max_tiles));
  HIPCHK(c, hipMemset(c->pool.mesh_stale(), 0, c->cfg.max_tiles));
  mesh_reset(c);   // the mesh goes with the map
  HIPCHK(c, hipMemset(c->d_state, 0, 64 * (kSlots + 1)));
  if (!keep_integrator_state) {
    // a cleared context behaves like a fresh one: both approximate sets as their constructor leaves them
    HIPCHK(c, hipMemset(c->d_start_set, 0, sizeof(uint64_t) << kSetBits));
    for (int t = 0; t < c->n_obs; ++t) {
      HIPCHK(c, hipMemset(c->d_observed_[t], 0, 2 * (sizeof(uint64_t) << kSetBits)));
      HIPCHK(c, hipMemcpy(c->d_observed_[t], &kObsPoison, 8, hipMemcpyHostToDevice));
    }
    const uint64_t poison = ~0ull;
    HIPCHK(c, hipMemcpy(c->d_start_set, &poison, 8, hipMemcpyHostToDevice));
    if (c->d_eo_plain) {
      HIPCHK(c, hipMemset(c->d_eo_plain, 0, sizeof(uint64_t) << kSetBits));
      HIPCHK(c, hipMemcpy(c->d_eo_plain, &poison, 8, hipMemcpyHostToDevice));
      HIPCHK(c, hipMemset(c->d_eo_committed, 0, 64));
      c->eo_frame_no = 0;
      c->eo_last_commit = nullptr;
    }
    c->start_offset = c->observed_offset = 0;
    c->reset_counter = 0;
    c->obs_tag = 0;
    c->obs_tag_lo = 1;
  }
  c->tiles_initialised = 0;
  for (auto& S : c->slot)
    if (S.h_snap) std::memset(S.h_snap, 0, sizeof(HostSnap));  // (the pool-growth trigger reads the snapshots' tile counts)
  c->fatal = false;
  return KS_OK;
}

int ks_clear(ks_ctx* c) {
  if (!c) return KS_ERR_INVALID_ARG;
  return clear_impl(c, false);
}

// ---- removal of blocks from the resident map (ks_k_remove.h) -------------------------------------------------
// What both entry points do first: refuse a context that holds no voxel data or has failed, complete the frames in flight —
// their statistics stay owed (c->owed is not touched: the trap of clear_impl) and the integrator's own state stays as they left
// it — and clear the byte plane the selection writes.
static int remove_begin(ks_ctx* c, const char* who, ks_remove_stats* stats) {
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (int rc = holds_voxels(c, who)) return rc;
  if (c->fatal) {
    c->err = std::string(who) + ": context is in a failed state (earlier pool/index error)";
    return KS_ERR_INVALID_ARG;
  }
  if (int rc = quiesce(c)) return rc;
  const size_t nt = c->tiles_initialised;
  if (int rc = c->rm_mark.reserve(c, nt, nt + nt / 2 + 64)) return rc;
  if (nt) HIPCHK(c, hipMemsetAsync(c->rm_mark, 0, nt, c->stream));
  return KS_OK;
}

// The tiles marked in c->rm_mark leave the map: the survivors above the new tile count move into the holes below it, the
// directory is rebuilt over the slots that remain, and the bookkeeping of the stored products follows the slots.
static int remove_tiles(ks_ctx* c, ks_remove_stats* stats) {
  hipStream_t st = c->stream;
  TileSnapshot snap(c);
  const uint32_t nt = snap.nt;
  const int sh = c->vps_shift;
  int rc;
  c->removed_blocks.clear();
  std::vector<uint8_t> mark(nt);
  if (nt) HIPCHK(c, hipMemcpyAsync(mark.data(), c->rm_mark, nt, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  uint32_t n_removed = 0;
  for (uint32_t s = 0; s < nt; ++s) n_removed += mark[s] != 0;
  const uint32_t nt_new = nt - n_removed;
  if (stats) {
    stats->tiles_resident = nt_new;
    stats->pool_capacity_tiles = c->cfg.max_tiles;
  }
  if (n_removed == 0) return KS_OK;
  c->nav_valid = false;   // slots move below and the navigation field does not follow
  drop_frontiers(c);      // ... nor do the frontier ids (§21)
  drop_rooms(c);          // ... nor the two planes of the rooms (§25)
  if ((rc = snap.fetch_keys(c))) return rc;
  // 1) what leaves: tile positions and blocks, ascending
  std::vector<uint64_t> gone_tiles;
  gone_tiles.reserve(n_removed);
  for (uint32_t s = 0; s < nt; ++s) {
    if (!mark[s]) continue;
    int t[3];
    snap.tile(s, t);
    gone_tiles.push_back(pack_coord3(t[0], t[1], t[2]));
  }
  std::sort(gone_tiles.begin(), gone_tiles.end());
  const std::vector<uint64_t> gone_blocks = blocks_of_tiles(gone_tiles, sh);
  // 2) every survivor at a slot >= nt_new moves into a hole < nt_new: there are as many of the one as of the other, and
  //    sources and destinations are disjoint
  std::vector<uint2> moves;
  for (uint32_t s = nt_new, hole = 0; s < nt; ++s) {
    if (mark[s]) continue;
    while (!mark[hole]) ++hole;
    moves.push_back(make_uint2(s, hole++));
  }
  if ((rc = c->rm_moves.reserve(c, moves.size(), moves.size() + moves.size() / 2 + 64))) return rc;
  // the blocks of the tiles that joined since the last mesh update enter the mesher's list now: their slots are renumbered below
  std::vector<uint64_t> fresh;
  if ((rc = snap.blocks(c, sh, c->mesh_tiles_seen, 0, &fresh))) return rc;
  // 3) move, rebuild the directory over [0, nt_new) (the sequence of grow_pool; table and pool stay where they are, so captured
  //    graphs stay valid), clear the flags of the vacated slots, set the persistent tile count
  const bool esdf = c->esdf_valid && c->esdf_tiles, obj = c->obj_valid && c->obj_tiles;
  if (!moves.empty()) {
    HIPCHK(c, hipMemcpyAsync(c->rm_moves, moves.data(), moves.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_remove_move, dim3((uint32_t)moves.size()), dim3(512), 0, st, c->pool, c->table.slot_keys, (const uint2*)c->rm_moves.get(),
                       esdf ? c->esdf_store.get() : (EsdfRecord*)nullptr, c->esdf_tiles, obj ? c->obj_ids.get() : (uint32_t*)nullptr, c->obj_tiles);
  }
  HIPCHK(c, hipMemsetAsync(c->table.ent, 0xff, ((size_t)c->table.mask + 1) * sizeof(TileEntry), st));
  if (nt_new) hipLaunchKernelGGL(k_rehash_tiles, dim3((nt_new + 255) / 256), dim3(256), 0, st, c->table, (const uint64_t*)c->table.slot_keys, nt_new);
  HIPCHK(c, hipMemsetAsync(c->pool.updated + nt_new, 0, n_removed, st));
  HIPCHK(c, hipMemsetAsync(c->pool.dirty + nt_new, 0, n_removed, st));
  HIPCHK(c, hipMemsetAsync(c->pool.mesh_stale() + nt_new, 0, n_removed, st));
  HIPCHK(c, hipMemcpyAsync(c->table.n_tiles, &nt_new, sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  c->tiles_initialised = nt_new;
  for (auto& S : c->slot)
    if (S.h_snap) S.h_snap->n_tiles = nt_new;   // (the pool-growth trigger reads the snapshots' tile counts)
  // 4) the stored products.  Mesh: the block list loses the blocks; the next update reports them and re-meshes what read them.
  {
    std::vector<uint64_t> all, kept;
    std::set_union(c->mesh_blocks.begin(), c->mesh_blocks.end(), fresh.begin(), fresh.end(), std::back_inserter(all));
    std::set_difference(all.begin(), all.end(), gone_blocks.begin(), gone_blocks.end(), std::back_inserter(kept));
    c->mesh_blocks.swap(kept);
    c->mesh_tiles_seen = nt_new;
    if (c->mesh_valid) {
      std::vector<uint64_t> both;
      std::set_union(c->mesh_removed.begin(), c->mesh_removed.end(), gone_blocks.begin(), gone_blocks.end(), std::back_inserter(both));
      c->mesh_removed.swap(both);
    }
  }
  // ESDF: records have moved with their tiles; the positions that lost their tile are stale positions of the next refresh
  if (c->esdf_valid) {
    std::vector<uint64_t> both;
    std::set_union(c->esdf_removed.begin(), c->esdf_removed.end(), gone_tiles.begin(), gone_tiles.end(), std::back_inserter(both));
    c->esdf_removed.swap(both);
    c->esdf_tiles = std::min(c->esdf_tiles, nt_new);
  }
  // objects: the records are the snapshot of the last update; the ids have moved with their tiles
  if (c->obj_valid) c->obj_tiles = std::min(c->obj_tiles, nt_new);
  words_to_triples(gone_blocks, &c->removed_blocks);
  if (stats) {
    stats->blocks_removed = gone_blocks.size();
    stats->tiles_removed = n_removed;
    stats->tiles_moved = moves.size();
  }
  return KS_OK;
}

int ks_remove_blocks(ks_ctx* c, const int32_t* idx, size_t n, ks_remove_stats* stats) {
  if (!c || (n && !idx)) return KS_ERR_INVALID_ARG;
  const int tpb = c->cfg.voxels_per_side / 8;
  const int lim = kTileBias / tpb;
  std::vector<uint64_t> keys;
  keys.reserve(n * tpb * tpb * tpb);
  for (size_t b = 0; b < n; ++b) {
    const int bx = idx[3 * b], by = idx[3 * b + 1], bz = idx[3 * b + 2];
    if (bx < -lim || bx >= lim || by < -lim || by >= lim || bz < -lim || bz >= lim) {
      c->err = "ks_remove_blocks: block index outside the packed tile-key range";
      return KS_ERR_INDEX_RANGE;
    }
    for (int z = 0; z < tpb; ++z)
      for (int y = 0; y < tpb; ++y)
        for (int x = 0; x < tpb; ++x) keys.push_back(pack_tile(bx * tpb + x, by * tpb + y, bz * tpb + z));
  }
  if (keys.size() >= (1ull << 31)) {
    c->err = "ks_remove_blocks: too many blocks for one call";
    return KS_ERR_INVALID_ARG;
  }
  int rc;
  if ((rc = remove_begin(c, "ks_remove_blocks", stats))) return rc;
  const uint32_t nt = c->tiles_initialised;
  if (!keys.empty() && nt) {
    if ((rc = c->rm_keys.reserve(c, keys.size(), keys.size() + keys.size() / 2))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->rm_keys, keys.data(), keys.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_remove_select_list, dim3((uint32_t)((keys.size() + 255) / 256)), dim3(256), 0, c->stream, c->table,
                       (const uint64_t*)c->rm_keys.get(), (uint32_t)keys.size(), nt, c->rm_mark.get());
  }
  return remove_tiles(c, stats);
}

int ks_remove_distant_blocks(ks_ctx* c, const float center[3], float max_distance_m, ks_remove_stats* stats) {
  if (!c || !center) return KS_ERR_INVALID_ARG;
  if (!std::isfinite(center[0]) || !std::isfinite(center[1]) || !std::isfinite(center[2]) || !(max_distance_m >= 0.0f) ||
      !std::isfinite(max_distance_m)) {
    c->err = "ks_remove_distant_blocks: the centre must be finite and max_distance_m finite and not negative";
    return KS_ERR_INVALID_ARG;
  }
  int rc;
  if ((rc = remove_begin(c, "ks_remove_distant_blocks", stats))) return rc;
  const uint32_t nt = c->tiles_initialised;
  if (nt) {
    RemoveRule R{};
    R.block_size = c->cfg.voxel_size * (float)c->cfg.voxels_per_side;
    R.cx = center[0], R.cy = center[1], R.cz = center[2];
    R.max_distance = max_distance_m;
    R.vps_shift = c->vps_shift;
    hipLaunchKernelGGL(k_remove_select_distance, dim3((nt + 255) / 256), dim3(256), 0, c->stream, (const uint64_t*)c->table.slot_keys, nt, R,
                       c->rm_mark.get());
  }
  return remove_tiles(c, stats);
}

int ks_removed_blocks(ks_ctx* c, int32_t* out_xyz, size_t cap, size_t* n) {
  return c ? copy_block_list(c, "ks_removed_blocks", c->removed_blocks, out_xyz, cap, n) : KS_ERR_INVALID_ARG;
}

// ---- fusing a submap at a rigid pose (ks_k_fuse.h) ---------------------------------------------------------------
int ks_fuse_default_config(ks_fuse_config* f) {
  if (!f) return KS_ERR_INVALID_ARG;
  f->min_weight = 1e-4f;
  f->pad = 0;
  f->max_workspace_bytes = 1ull << 30;
  return KS_OK;
}

namespace {
constexpr uint64_t kFuseTileBytes = (uint64_t)kTileVoxels * 128 + 16;   // the tile, its key, its count, its idx entry
struct Pose64 {
  double w, v[3], t[3];
};
void cross64(const double a[3], const double b[3], double out[3]) {
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}
// r = (p + (2 w) (v x p)) + 2 (v x (v x p)), in this form
void rotate64(const Pose64& T, const double p[3], double r[3]) {
  double uv[3], c2[3];
  cross64(T.v, p, uv);
  cross64(T.v, uv, c2);
  for (int k = 0; k < 3; ++k) r[k] = (p[k] + (2.0 * T.w) * uv[k]) + 2.0 * c2[k];
}
// The destination tiles the source tiles can reach: a destination voxel is touched only if the lowest corner of its sample lies in
// a resident source tile s, i.e. its point lies in the cube vs * [8 s + 0.5, 8 s + 8.5)^3; the cube's corners through T_D_S (f64)
// bound the voxel's centre, and one voxel on every side covers what f32 rounds differently.  Ascending, unique.
int fuse_candidates(ks_ctx* d, const std::vector<uint64_t>& src_keys, const Pose64& T_D_S, std::vector<uint64_t>* out) {
  const double vs = (double)d->cfg.voxel_size;
  out->clear();
  out->reserve(src_keys.size() * 8);
  for (uint64_t key : src_keys) {
    int s[3];
    unpack_tile(key, s[0], s[1], s[2]);
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int k = 0; k < 8; ++k) {
      const double p[3] = {vs * (8.0 * s[0] + 0.5 + 8.0 * (k & 1)), vs * (8.0 * s[1] + 0.5 + 8.0 * ((k >> 1) & 1)), vs * (8.0 * s[2] + 0.5 + 8.0 * (k >> 2))};
      double r[3];
      rotate64(T_D_S, p, r);
      for (int a = 0; a < 3; ++a) {
        const double c = r[a] + T_D_S.t[a];
        lo[a] = std::min(lo[a], c);
        hi[a] = std::max(hi[a], c);
      }
    }
    int t0[3], t1[3];
    for (int a = 0; a < 3; ++a) {
      const double v0 = std::floor(lo[a] / vs - 0.5) - 1.0, v1 = std::ceil(hi[a] / vs - 0.5) + 1.0;
      const double a0 = std::floor(v0 / 8.0), a1 = std::floor(v1 / 8.0);
      if (!(a0 >= -(double)kTileBias) || !(a1 < (double)kTileBias)) {
        d->err = "ks_fuse_map: a candidate tile leaves the packed tile-key range";
        return KS_ERR_INDEX_RANGE;
      }
      t0[a] = (int)a0;
      t1[a] = (int)a1;
    }
    for (int x = t0[0]; x <= t1[0]; ++x)
      for (int y = t0[1]; y <= t1[1]; ++y)
        for (int z = t0[2]; z <= t1[2]; ++z) out->push_back(pack_tile(x, y, z));
  }
  sort_unique(*out);
  return KS_OK;
}
}  // namespace

int ks_fuse_map(ks_ctx* d, ks_ctx* s, const float T[7], const ks_fuse_config* f, ks_fuse_stats* stats) {
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!d || !s || !T || !f) return KS_ERR_INVALID_ARG;
  auto refuse = [&](const char* why) {
    d->err = std::string("ks_fuse_map: ") + why;
    return KS_ERR_INVALID_ARG;
  };
  if (d == s) return refuse("dst and src are the same context (use a second context)");
  if (d->cfg.device_id != s->cfg.device_id) return refuse("the two contexts live on different devices");
  if (std::memcmp(&d->cfg.voxel_size, &s->cfg.voxel_size, sizeof(float)) != 0) return refuse("the two contexts differ in voxel_size");
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(T[k])) return refuse("the pose must be finite");
  const double qn = std::sqrt((double)T[0] * T[0] + (double)T[1] * T[1] + (double)T[2] * T[2] + (double)T[3] * T[3]);
  if (!(qn > 0.0)) return refuse("the quaternion is zero");
  if (!std::isfinite(f->min_weight) || !(f->min_weight > 0.0f)) return refuse("min_weight must be a finite positive number");
  int rc;
  if ((rc = holds_voxels(d, "ks_fuse_map"))) return rc;
  if (s->shard_export) {
    d->err = "ks_fuse_map: src is a marcher context of ks_integrate_round_exact and holds no voxel data";
    return KS_ERR_UNSUPPORTED;
  }
  if (d->fatal || s->fatal) return refuse("a context is in a failed state (earlier pool/index error)");
  // the frames in flight of both contexts; their statistics stay owed (c->owed is not touched)
  if ((rc = quiesce(d))) return rc;
  if ((rc = quiesce(s))) {
    d->err = "ks_fuse_map: src: " + s->err;
    return rc;
  }
  // 1. the inverse pose, f64, rounded to f32 at the end
  Pose64 T_D_S{(double)T[0] / qn, {(double)T[1] / qn, (double)T[2] / qn, (double)T[3] / qn}, {(double)T[4], (double)T[5], (double)T[6]}};
  Pose64 inv{T_D_S.w, {-T_D_S.v[0], -T_D_S.v[1], -T_D_S.v[2]}, {0, 0, 0}};
  {
    double r[3];
    rotate64(inv, T_D_S.t, r);
    for (int k = 0; k < 3; ++k) inv.t[k] = -r[k];
  }
  FuseView V{};
  V.T.w = (float)inv.w;
  V.T.v = {(float)inv.v[0], (float)inv.v[1], (float)inv.v[2]};
  V.T.t = {(float)inv.t[0], (float)inv.t[1], (float)inv.t[2]};
  V.voxel_size = d->cfg.voxel_size;
  V.voxel_size_inv = d->voxel_size_inv;
  V.min_weight = f->min_weight;
  V.n_src_tiles = s->tiles_initialised;
  TileSnapshot snap(s);
  if (stats) stats->tiles_source = snap.nt;
  if (snap.nt == 0) return KS_OK;
  if ((rc = snap.fetch_keys(s))) {
    d->err = "ks_fuse_map: src: " + s->err;
    return rc;
  }
  std::vector<uint64_t> cand;
  if ((rc = fuse_candidates(d, snap.keys, T_D_S, &cand))) return rc;
  const size_t nc = cand.size();
  if (stats) stats->tiles_candidate = nc;
  const size_t per_chunk = (size_t)std::min<uint64_t>(f->max_workspace_bytes / kFuseTileBytes, nc);
  if (per_chunk == 0) {
    if (stats) stats->workspace_bytes = kFuseTileBytes;
    d->err = "ks_fuse_map: max_workspace_bytes is below what one tile needs";
    return KS_ERR_UNSUPPORTED;
  }
  if (stats) stats->workspace_bytes = per_chunk * kFuseTileBytes;
  if ((rc = d->fuse_ws.reserve(d, per_chunk * kTileVoxels * 8, per_chunk * kTileVoxels * 8))) return rc;
  if ((rc = d->fuse_keys.reserve(d, 2 * per_chunk, 2 * per_chunk))) return rc;
  if ((rc = d->fuse_u32.reserve(d, 3 * per_chunk + 1, 3 * per_chunk + 1))) return rc;
  hipStream_t st = d->stream;
  const uint32_t tiles_before = d->tiles_initialised;
  std::vector<uint32_t> counts, offs, idx;
  std::vector<uint64_t> ukeys;
  for (size_t first = 0; first < nc; first += per_chunk) {
    const size_t m = std::min(per_chunk, nc - first);
    uint64_t* d_cand = d->fuse_keys;
    uint64_t* d_ukeys = d->fuse_keys + per_chunk;
    uint32_t* d_counts = d->fuse_u32;
    uint32_t* d_offs = d->fuse_u32 + per_chunk;
    HIPCHK(d, hipMemcpyAsync(d_cand, cand.data() + first, m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_fuse_resample, dim3((uint32_t)m), dim3(512), 0, st, s->table, s->pool, V, (const uint64_t*)d_cand, d->fuse_ws.get(), d_counts);
    counts.resize(m);
    HIPCHK(d, hipMemcpyAsync(counts.data(), d_counts, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(d, hipStreamSynchronize(st));
    HIPCHK(d, hipGetLastError());
    if (stats) stats->chunks += 1;
    // the tiles that hold a touched voxel go to the existing insertion and merge: one incoming tile per key, picked by its index
    ukeys.clear(), offs.clear(), idx.clear();
    uint64_t voxels = 0;
    for (size_t i = 0; i < m; ++i) {
      if (!counts[i]) continue;
      offs.push_back((uint32_t)ukeys.size());
      ukeys.push_back(cand[first + i]);
      idx.push_back((uint32_t)i);
      voxels += counts[i];
    }
    const size_t nu = ukeys.size();
    if (nu == 0) continue;
    offs.push_back((uint32_t)nu);
    uint32_t* d_idx = d_offs + (nu + 1);
    HIPCHK(d, hipMemcpyAsync(d_ukeys, ukeys.data(), nu * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIPCHK(d, hipMemcpyAsync(d_offs, offs.data(), (nu + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(d, hipMemcpyAsync(d_idx, idx.data(), nu * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if ((rc = insert_tiles(d, d_ukeys, nu))) return rc;
    const uint4* in = d->fuse_ws.get();
    switch (d->cfg.color_mode) {
      case KS_COLOR_MODE_COLOR:
        hipLaunchKernelGGL(k_merge_tiles<KS_COLOR_MODE_COLOR>, dim3((uint32_t)nu), dim3(512), 0, st, d->table, d->pool, (const uint64_t*)d_ukeys,
                           (const uint32_t*)d_offs, (const uint32_t*)d_idx, in, d->cfg.max_weight, (const uint32_t*)d->d_label_lut);
        break;
      case KS_COLOR_MODE_SEMANTIC:
        hipLaunchKernelGGL(k_merge_tiles<KS_COLOR_MODE_SEMANTIC>, dim3((uint32_t)nu), dim3(512), 0, st, d->table, d->pool, (const uint64_t*)d_ukeys,
                           (const uint32_t*)d_offs, (const uint32_t*)d_idx, in, d->cfg.max_weight, (const uint32_t*)d->d_label_lut);
        break;
      default:
        hipLaunchKernelGGL(k_merge_tiles<KS_COLOR_MODE_SEMANTIC_PROBABILITY>, dim3((uint32_t)nu), dim3(512), 0, st, d->table, d->pool,
                           (const uint64_t*)d_ukeys, (const uint32_t*)d_offs, (const uint32_t*)d_idx, in, d->cfg.max_weight,
                           (const uint32_t*)d->d_label_lut);
        break;
    }
    // what k_merge_tiles leaves to its callers: both sync flags of the tiles it folded into
    hipLaunchKernelGGL(k_fuse_flag, dim3((uint32_t)((nu + 255) / 256)), dim3(256), 0, st, d->table, d->pool, (const uint64_t*)d_ukeys, (uint32_t)nu,
                       d->tiles_initialised);
    HIPCHK(d, hipStreamSynchronize(st));
    HIPCHK(d, hipGetLastError());
    if (stats) {
      stats->tiles_touched += nu;
      stats->voxels_fused += voxels;
      stats->tiles_allocated = d->tiles_initialised - tiles_before;
    }
  }
  return KS_OK;
}

int ks_clear_voxels(ks_ctx* c) {
  if (!c) return KS_ERR_INVALID_ARG;
  return clear_impl(c, true);
}

int ks_flush(ks_ctx* c, ks_frame_stats* stats) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const int rc = flush_pending(c);
  deliver_stats(c, stats);
  return rc;
}

int ks_synchronize(ks_ctx* c) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (int rc = quiesce(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KS_OK;
}

void* ks_stream(ks_ctx* c) { return c ? (void*)c->stream : nullptr; }

#ifdef KS_STATS
// diagnostics build only: read (and clear) the k_test counters
int ks_debug_test_stats(unsigned long long* out16) {
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_test_stats), 16 * sizeof(unsigned long long)) != hipSuccess) return KS_ERR_HIP;
  unsigned long long z[16] = {0};
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_test_stats), z, sizeof(z)) != hipSuccess) return KS_ERR_HIP;
  return KS_OK;
}
#endif

int ks_early_out_iterations(ks_ctx* c, uint64_t* frames, uint64_t* iterations) {
  if (!c) return KS_ERR_INVALID_ARG;
  if (frames) *frames = c->eo_frames;
  if (iterations) *iterations = c->eo_iterations;
  return KS_OK;
}

int ks_early_out_stats(ks_ctx* c, uint64_t out[5]) {
  if (!c || !out) return KS_ERR_INVALID_ARG;
  out[0] = c->eo_frames;
  out[1] = c->eo_iterations;
  out[2] = c->eo_fallbacks.load(std::memory_order_relaxed);
  out[3] = (c->eo_device && !c->eo_device_off) ? 1 : 0;
  out[4] = (c->exact_early_out && c->cfg.pipeline_frames > 0) ? 1 : 0;
  return KS_OK;
}

int ks_update_stats(ks_ctx* c, uint64_t out[4]) {
  if (!c || !out) return KS_ERR_INVALID_ARG;
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!c->d_xl_hdr) return KS_OK;
  if (int rc = quiesce(c)) return rc;
  if (c->stream_xlong) HIPCHK(c, hipStreamSynchronize(c->stream_xlong));
  XlHeader h;
  HIPCHK(c, hipMemcpy(&h, c->d_xl_hdr, sizeof(h), hipMemcpyDeviceToHost));
  out[0] = h.tot_walked;
  out[1] = h.tot_fallback;
  out[2] = h.tot_chunks;
  out[3] = h.tot_replayed;
  return KS_OK;
}

int ks_pipeline_shape(ks_ctx* c, int32_t out[4]) {
  if (!c || !out) return KS_ERR_INVALID_ARG;
  out[0] = c->cfg.pipeline_frames;
  out[1] = c->n_slots;
  out[2] = c->batch;
  out[3] = c->n_march;
  return KS_OK;
}

int ks_tail_batch_stats(ks_ctx* c, uint64_t out[4]) {
  if (!c || !out) return KS_ERR_INVALID_ARG;
  for (int i = 0; i < 4; ++i) out[i] = c->tb_stats[i];
  return KS_OK;
}

int ks_tail_batch_rule(const uint32_t* err, const uint64_t* n_pairs, int32_t nb, int32_t marcher, int32_t profiling, uint64_t apply_runs_min_pairs) {
  if (!err || !n_pairs || nb < 0 || nb > kBatchMax) return KS_ERR_INVALID_ARG;
  unsigned long long np[kBatchMax];
  for (int k = 0; k < nb; ++k) np[k] = n_pairs[k];
  return tail_batch_rule(err, np, nb, marcher != 0, profiling, apply_runs_min_pairs, ~0ull) ? 1 : 0;
}

int ks_stream_plan(ks_ctx* c, int32_t out[8]) {
  if (!c || !out) return KS_ERR_INVALID_ARG;
  const StreamPlan& P = c->plan;
  out[0] = P.budget;
  out[1] = P.distinct;
  out[2] = P.n_march;
  out[3] = P.long_own ? 1 : 0;
  out[4] = !c->xlong ? -1 : P.xlong_own ? 1 : 0;
  out[5] = P.march_own ? 1 : 0;
  out[6] = P.tail_own ? 1 : 0;
  out[7] = c->n_streams;   // streams the context holds (= out[1])
  return KS_OK;
}

int ks_seed_launch_shape(int32_t order_mode, int32_t phase_growth, uint64_t cap_points, uint32_t* out, int32_t max_phases) {
  if (order_mode < KS_ORDER_MIXED || order_mode > KS_ORDER_MIXED_1024_GROUPS || phase_growth < 16 || phase_growth > 4096 || cap_points == 0 ||
      cap_points > kObsMaxPoints || (max_phases > 0 && !out))
    return KS_ERR_INVALID_ARG;
  const std::vector<SeedPhase> ph = seed_launch_shape(order_mode, phase_growth, std::max<size_t>((size_t)cap_points, 1024));   // (ensure_points: a slot holds 1024 points at least)
  for (size_t j = 0; j < ph.size() && (int64_t)j < (int64_t)max_phases; ++j) {
    out[3 * j] = ph[j].g0;
    out[3 * j + 1] = ph[j].g1;
    out[3 * j + 2] = ph[j].item_cap;
  }
  return (int)ph.size();
}

int ks_profile_enable(ks_ctx* c, int level) {
  if (!c || level < 0 || level > 2) return KS_ERR_INVALID_ARG;
  c->profiling = level;
  return KS_OK;
}

int ks_profile_get(ks_ctx* c, ks_profile* out, int reset) {
  if (!c || !out) return KS_ERR_INVALID_ARG;
  if (int rc = quiesce(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < kProfSets; ++i) resolve_prof(c, i);
  *out = c->prof;
  if (reset) c->prof = ks_profile{};
  return KS_OK;
}

}  // extern "C"
