// C ABI of libcgmr.so (include/cgmr.h): context management and the Gauss-Newton driver.
// Compiled with hipcc; contains no kernels (those live in gn_kernels.hip / matcher_kernels.hip).
#include "cgmr_ctx.h"
#include "dl_device.h"
#include "factor_model.h"
#include "gnc_device.h"
#include "gn_host.h"
#include "init_device.h"
#include "lm_device.h"
#include "pcm_device.h"
#include "tr_device.h"

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

namespace cgmr {

double wall_s() {
  using namespace std::chrono;
  return duration_cast<duration<double>>(steady_clock::now().time_since_epoch()).count();
}

int set_err(cgmr_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

#define HIP_TRY(ctx, call)                                                                      \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) return set_err(ctx, CGMR_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

int side_stream(cgmr_ctx* ctx) {
  if (ctx->side) return 0;
  // (default priority.  Round 4 tried the lowest priority here and the highest for the context's stream -- the batches as
  // gap fillers of the solve's dependent chain of small launches --: with eight robots on one device a starved batch held
  // up its own robot's next structure upload, optimize(5) 2.57 -> 4.49 ms in the loopback; without peers on the device no
  // gain either way.)
  HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
  HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->side_fork, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->side_tail, hipEventDisableTiming));
  return 0;
}

int side_fork(cgmr_ctx* ctx) {
  int rc = side_stream(ctx);
  if (rc) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->side_fork, ctx->stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->side, ctx->side_fork, 0));
  return 0;
}

int side_mark(cgmr_ctx* ctx) {
  HIP_TRY(ctx, hipEventRecord(ctx->side_tail, ctx->side));
  ctx->side_busy = true;
  return 0;
}

int side_join_host(cgmr_ctx* ctx) {
  if (!ctx->side_busy) return 0;
  HIP_TRY(ctx, hipEventSynchronize(ctx->side_tail));
  ctx->side_busy = false;
  return 0;
}

int side_join_stream(cgmr_ctx* ctx, hipStream_t st) {
  if (!ctx->side_busy) return 0;
  HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->side_tail, 0));
  return 0;
}

// An arena that has to grow is not freed on the spot: hipFree waits for the whole device -- every stream of every context
// of the process, e.g. the other robots' batches on their side streams -- and work queued on this context's streams may
// still read the old block.  The old block goes to the context's graveyard (freed with the context); the arena at least
// doubles, so the graveyard never holds more than the live blocks do (sized for 288 GB of HBM, not for thrift).
int arena_reserve(cgmr_ctx* ctx, Arena& A, size_t bytes) {
  if (bytes <= A.cap) return 0;
  if (A.ptr) { ctx->graveyard.push_back({A.ptr, nullptr}); A.ptr = nullptr; }
  size_t want = std::max(bytes + bytes / 2, 2 * A.cap) + (1 << 20);
  A.cap = 0;
  hipError_t e = hipMalloc((void**)&A.ptr, want);
  if (e != hipSuccess) return set_err(ctx, CGMR_E_ALLOC, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
  A.cap = want;
  return 0;
}

int pinned_reserve(cgmr_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->pinned_cap) return 0;
  if (ctx->pinned) { (void)hipStreamSynchronize(ctx->stream); (void)side_join_host(ctx); (void)hipHostFree(ctx->pinned); ctx->pinned = nullptr; ctx->pinned_cap = 0; }
  size_t want = std::max(2 * bytes, (size_t)4 << 20);      // (page-locking is slow and a robot's graph grows every round: double, never less than 4 MB)
  hipError_t e = hipHostMalloc((void**)&ctx->pinned, want, hipHostMallocDefault);
  if (e != hipSuccess) return set_err(ctx, CGMR_E_ALLOC, "hipHostMalloc(%zu): %s", want, hipGetErrorString(e));
  ctx->pinned_cap = want;
  return 0;
}

int pinned_mask_reserve(cgmr_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->pinned_mask_cap) return 0;
  if (ctx->pinned_mask) { (void)hipStreamSynchronize(ctx->stream); (void)side_join_host(ctx); (void)hipHostFree(ctx->pinned_mask); ctx->pinned_mask = nullptr; ctx->pinned_mask_cap = 0; }
  size_t want = bytes + bytes / 2 + 4096;
  hipError_t e = hipHostMalloc((void**)&ctx->pinned_mask, want, hipHostMallocDefault);
  if (e != hipSuccess) return set_err(ctx, CGMR_E_ALLOC, "hipHostMalloc(%zu): %s", want, hipGetErrorString(e));
  ctx->pinned_mask_cap = want;
  return 0;
}

struct BlobLayout {
  size_t off = 0;
  template <typename T>
  size_t add(size_t count) {
    off = (off + 15) & ~size_t(15);
    size_t o = off;
    off += count * sizeof(T);
    return o;
  }
};

// AnalyzeHooks::blocks_ready of a context's analysis: what the assembly lists depend on goes to the device as soon as it is
// final (vperm, the edge list, the off-diagonal blocks' rows / columns / column starts: one copy from a pinned block of its own)
// and the device builds the lists (gn_structure.hip) underneath the rest of the host's analysis.
int gn_upload_early(cgmr_ctx* ctx, const Symbolic& S, const int32_t* ef, const int32_t* et, const int32_t* offbase) {
  const size_t nV = (size_t)S.nV, nE = (size_t)S.nE, nb = (size_t)S.nb, nf = (size_t)S.nf, nkeys = nf + nb;
  BlobLayout B;
  const size_t o_vperm = B.add<int32_t>(nV), o_ef = B.add<int32_t>(nE), o_et = B.add<int32_t>(nE), o_orow = B.add<int32_t>(nb),
               o_ocol = B.add<int32_t>(nb), o_obase = B.add<int32_t>(nf + 1);
  const size_t up_bytes = (B.off + 255) & ~size_t(255);
  B.off = up_bytes;
  const size_t o_asmp = B.add<int32_t>(nkeys + 1), o_asms = B.add<int32_t>(3 * nE + 4), o_cnt = B.add<int32_t>(nkeys + 4),
               o_ekey = B.add<int32_t>(nE), o_long = B.add<int32_t>(3 * nE / 16 + 2), o_tmp = B.add<int32_t>(3 * nE + 4);
  // whatever still reads the previous structure on the side stream (a batch of condensed-graph passes) comes first
  int rc = side_join_stream(ctx, ctx->stream);
  if (rc) return rc;
  rc = arena_reserve(ctx, ctx->st_arena, B.off + 256);
  if (rc) return rc;
  if (!ctx->ev_st_copied) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_st_copied, hipEventDisableTiming));
  else HIP_TRY(ctx, hipEventSynchronize(ctx->ev_st_copied));   // (the previous copy out of the staging block: long done)
  if (up_bytes > ctx->pinned_st_cap) {
    if (ctx->pinned_st) { (void)hipHostFree(ctx->pinned_st); ctx->pinned_st = nullptr; ctx->pinned_st_cap = 0; }
    // (page-locking is slow and a robot's graph grows every round: double, and never less than 2 MB)
    const size_t want = std::max(2 * up_bytes, (size_t)2 << 20);
    hipError_t e = hipHostMalloc((void**)&ctx->pinned_st, want, hipHostMallocDefault);
    if (e != hipSuccess) return set_err(ctx, CGMR_E_ALLOC, "hipHostMalloc(%zu): %s", want, hipGetErrorString(e));
    ctx->pinned_st_cap = want;
  }
  char* h = ctx->pinned_st;
  host_run_tasks(4, [&](int task) {
    switch (task) {
      case 0: memcpy(h + o_ef, ef, 4 * nE); break;
      case 1: memcpy(h + o_et, et, 4 * nE); break;
      case 2: memcpy(h + o_orow, S.off_row.data(), 4 * nb); memcpy(h + o_obase, offbase, 4 * (nf + 1)); break;
      default: memcpy(h + o_ocol, S.off_col.data(), 4 * nb); memcpy(h + o_vperm, S.vperm.data(), 4 * nV); break;
    }
  });
  char* d = ctx->st_arena.ptr;
  HIP_TRY(ctx, hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(ctx->ev_st_copied, ctx->stream));
  cgmr_ctx::StView& V = ctx->st_view;
  V.vperm = (int32_t*)(d + o_vperm); V.ef = (int32_t*)(d + o_ef); V.et = (int32_t*)(d + o_et);
  V.off_row = (int32_t*)(d + o_orow); V.off_col = (int32_t*)(d + o_ocol); V.offbase = (int32_t*)(d + o_obase);
  V.asm_ptr = (int32_t*)(d + o_asmp); V.asm_src = (int32_t*)(d + o_asms);
  V.fresh = true;
  AsmBuild A;
  A.nE = S.nE; A.nf = S.nf; A.nb = S.nb;
  A.vperm = V.vperm; A.ef = V.ef; A.et = V.et; A.off_row = V.off_row; A.offbase = (const int32_t*)(d + o_obase);
  A.asm_ptr = V.asm_ptr; A.asm_src = V.asm_src; A.ekey = (int32_t*)(d + o_ekey); A.cnt = (int32_t*)(d + o_cnt);
  A.longlist = (int32_t*)(d + o_long); A.tmp = (int32_t*)(d + o_tmp);
  launch_build_asm(ctx->stream, A);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

// Lay out and upload the structure arrays the host made; point GnDevice into the arena.  vperm, the edge list, the off-diagonal
// blocks and the assembly lists are on the device already (gn_upload_early, which S's analysis called: ctx->st_view); the row
// maps, the destinations and the work records are made there from what goes up here (k_build_maps).
int gn_upload(cgmr_ctx* ctx, const Symbolic& S, int iters) {
  cgmr_ctx::StView& V = ctx->st_view;
  if (S.nf == 0) V = cgmr_ctx::StView();                    // (no column: the analysis ends before its hook, and no pass reads these)
  else if (!V.fresh) return set_err(ctx, CGMR_E_INVALID, "structure upload of an analysis without its device pass (AnalyzeHooks::blocks_ready)");
  V.fresh = false;
  // the factor kernels keep row positions (own columns + border rows) in 16-bit LDS maps
  if (3 * (int64_t)S.max_ns + kFrontW > 32767)
    return set_err(ctx, CGMR_E_INVALID, "a front has %d border poses; at most %d are supported", S.max_ns, (32767 - kFrontW) / 3);
  GnDevice& D = ctx->gn;
  D.nV = S.nV; D.nE = S.nE; D.nf = S.nf; D.nb = S.nb;
  D.nfronts = (int)S.fronts.size();
  D.nlevels = (int)S.gn_level_ptr.size() - 1;           // Gauss-Newton levels: without the top block
  D.h_level_ptr = S.gn_level_ptr;
  D.nlevels_full = (int)S.level_ptr.size() - 1;
  D.h_flevel_ptr = S.level_ptr;
  const std::vector<int32_t>& LF = S.gn_level_fronts;
  const Switches& sw = ctx->sw;
  // sizing pass: work records (one per front and row chunk) and update tiles per level fix the blob layout
  D.h_tile_ptr.assign(D.nlevels + 1, 0);
  D.h_work_ptr.assign(D.nlevels + 1, 0);
  D.h_level_chrows.assign(D.nlevels, 1);
  D.h_level_leaf.assign(D.nlevels, 1);
  D.h_level_chunk.assign(D.nlevels, kChunkRows);
  D.h_level_mergeable.assign(D.nlevels, 1);
  // update tiles run in the launch the schedule gave their front (sched_t: its own level or, with slack, a later one)
  std::vector<std::vector<int32_t>> sched(D.nlevels);
  for (int q = 0; q < (int)LF.size(); q++) {
    const FrontDesc& F = S.fronts[LF[q]];
    if (F.ns > 0) sched[std::min(F.sched_t, D.nlevels - 1)].push_back(LF[q]);
  }
  for (auto& v : sched) std::sort(v.begin(), v.end());
  // a front's first work record (the update tiles address the front through it) and its record count (0: top block), for k_build_maps
  std::vector<int32_t> rec0_of(2 * S.fronts.size(), 0);
  for (size_t f = 0; f < S.fronts.size(); f++) rec0_of[2 * f] = -1;
  for (int l = 0; l < D.nlevels; l++) {
    for (int q = S.gn_level_ptr[l]; q < S.gn_level_ptr[l + 1]; q++)
      if (S.fronts[LF[q]].nchild > 0) D.h_level_leaf[l] = 0;
    // a level of leaves has its own chunk length (kLeafChunkRows)
    int chunk_rows = D.h_level_leaf[l] ? sw.leaf_chunk : sw.mid_chunk;
    // the few fronts of an upper level (an idle chip): shorter chunks = more workgroups per front, each with less of the
    // panel to pull in on its own (a lone workgroup fetches cold data at 10-25 bytes per clock) -- and few extra records
    if (!D.h_level_leaf[l] && S.gn_level_ptr[l + 1] - S.gn_level_ptr[l] <= sw.top_chunk_fronts) chunk_rows = std::min(chunk_rows, sw.top_chunk);
    D.h_level_chunk[l] = chunk_rows;
    int nwork = 0;
    for (int q = S.gn_level_ptr[l]; q < S.gn_level_ptr[l + 1]; q++) {
      const int r = 3 * S.fronts[LF[q]].ns;
      const int nchunk = std::max(1, (r + chunk_rows - 1) / chunk_rows);
      rec0_of[2 * LF[q]] = D.h_work_ptr[l] + nwork;
      rec0_of[2 * LF[q] + 1] = nchunk;
      nwork += nchunk;
      D.h_level_chrows[l] = std::max(D.h_level_chrows[l], std::min(r, chunk_rows) + 1);
    }
    int xload[8] = {0, 0, 0, 0, 0, 0, 0, 0};                     // update tiles per XCD (see the tile list below)
    for (int f : sched[l]) {
      if (S.fronts[f].nchild > kWorkChildren) D.h_level_mergeable[l] = 0;
      const int T = (3 * S.fronts[f].ns + 31) / 32;
      *std::min_element(xload, xload + 8) += T * (T + 1) / 2;
    }
    D.h_tile_ptr[l + 1] = D.h_tile_ptr[l] + 8 * *std::max_element(xload, xload + 8);
    D.h_work_ptr[l + 1] = D.h_work_ptr[l] + nwork;
  }
  const size_t n_tiles = (size_t)D.h_tile_ptr[D.nlevels], n_work = (size_t)D.h_work_ptr[D.nlevels];
  BlobLayout B;
  size_t o_fronts = B.add<FrontDesc>(S.fronts.size());
  size_t o_fronts_lv = B.add<FrontDesc>(S.fronts.size());   // the same descriptors in level order: the solves index them by workgroup
  size_t o_rows = B.add<int32_t>(S.rows.size());
  size_t o_children = B.add<int32_t>(S.children.size());
  size_t o_lf = B.add<int32_t>(S.level_fronts.size());
  size_t o_tiles = B.add<int32_t>(3 * n_tiles);
  size_t o_rec0 = B.add<int32_t>(rec0_of.size());
  size_t o_tf = B.add<int32_t>(S.top_fronts.size()), o_tc = B.add<int32_t>(S.top_children.size()), o_tb = B.add<int32_t>(S.top_blocks.size());
  size_t blob_bytes = (B.off + 255) & ~size_t(255);
  // numeric work space
  BlobLayout N;
  N.off = blob_bytes;
  size_t o_term = N.add<double>((size_t)34 * S.nE);
  size_t o_A = N.add<double>((size_t)9 * (S.nf + S.nb));
  size_t o_b = N.add<double>((size_t)3 * S.nf);
  size_t o_y = N.add<double>((size_t)3 * S.nf);
  size_t o_x = N.add<double>((size_t)3 * S.nf);
  size_t o_u = N.add<double>((size_t)3 * S.rows.size() + 3);
  size_t o_L = N.add<double>((size_t)S.L_doubles + 1);
  size_t o_U = N.add<double>((size_t)S.U_doubles + 1);
  size_t o_pan = N.add<double>((size_t)S.pan_doubles + 2);
  size_t o_chi = N.add<double>((size_t)iters + 2);
  size_t o_status = N.add<int>(4);
  size_t o_ready = N.add<int>(S.fronts.size() + 4);
  size_t o_cmask = N.add<uint8_t>((size_t)S.nf + 16);
  // (device-made: k_build_maps)
  size_t o_rel = N.add<int32_t>((size_t)S.n_rel + 4), o_inv = N.add<int32_t>((size_t)S.n_inv + 4);
  size_t o_bdst = N.add<int32_t>((size_t)S.nf + S.nb + 4), o_rdst = N.add<int32_t>((size_t)S.nf + 4);
  size_t o_work = N.add<WorkRec>(n_work + 1);
  size_t total = N.off + 256;
  int rc = arena_reserve(ctx, ctx->gn_arena, total);
  if (rc) return rc;
  rc = pinned_reserve(ctx, blob_bytes);
  if (rc) return rc;
  char* h = ctx->pinned;
  auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes) memcpy(h + off, src, bytes); };
  // staging: independent pieces on the analysis' helper threads
  host_run_tasks(6, [&](int task) {
    switch (task) {
      case 0: {                                                  // update tiles, level by level
        int32_t* tiles = reinterpret_cast<int32_t*>(h + o_tiles);
        // Update tiles of one front sit 8 apart in the launch: workgroup b runs on XCD b % 8 (observed; speed only), so
        // the tiles that share the front's L21 rows share one L2 instead of fetching them into up to eight.  A front goes
        // to the XCD with the fewest tiles so far; the shorter queues are padded with empty entries (rec = -1).
        for (int l = 0; l < D.nlevels; l++) {
          int32_t* tl = tiles + 3 * (size_t)D.h_tile_ptr[l];
          const int slots = D.h_tile_ptr[l + 1] - D.h_tile_ptr[l];
          for (int k = 0; k < slots; k++) { tl[3 * k] = -1; tl[3 * k + 1] = 0; tl[3 * k + 2] = 0; }
          int xload[8] = {0, 0, 0, 0, 0, 0, 0, 0};
          for (int f : sched[l]) {
            const int T = (3 * S.fronts[f].ns + 31) / 32;
            const int x = (int)(std::min_element(xload, xload + 8) - xload);
            for (int ti = 0; ti < T; ti++)
              for (int tj = 0; tj <= ti; tj++) {
                int32_t* e = tl + 3 * (size_t)(8 * xload[x]++ + x);
                e[0] = rec0_of[2 * f]; e[1] = ti; e[2] = tj;
              }
          }
        }
        break;
      }
      case 1:
        put(o_rec0, rec0_of.data(), rec0_of.size() * 4);
        put(o_children, S.children.data(), S.children.size() * 4);
        break;
      case 2:
        put(o_fronts, S.fronts.data(), S.fronts.size() * sizeof(FrontDesc));
        break;
      case 3: {
        FrontDesc* lv = reinterpret_cast<FrontDesc*>(h + o_fronts_lv);       // Gauss-Newton level order (the backward solve's index)
        for (size_t q = 0; q < S.fronts.size(); q++) {
          if (q < LF.size()) lv[q] = S.fronts[LF[q]];
          else memset(&lv[q], 0, sizeof(FrontDesc));             // fronts of the top block: not addressed through this table
        }
        break;
      }
      case 4:
        put(o_lf, S.level_fronts.data(), S.level_fronts.size() * 4);
        put(o_tf, S.top_fronts.data(), S.top_fronts.size() * 4);
        put(o_tc, S.top_children.data(), S.top_children.size() * 4);
        put(o_tb, S.top_blocks.data(), S.top_blocks.size() * 4);
        break;
      default:
        put(o_rows, S.rows.data(), S.rows.size() * 4);
        break;
    }
  });
  char* d = ctx->gn_arena.ptr;
  // a batch on the side stream still reads the structure this upload replaces
  rc = side_join_stream(ctx, ctx->stream);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(d, h, blob_bytes, hipMemcpyHostToDevice, ctx->stream));
  D.fronts = (FrontDesc*)(d + o_fronts);
  D.fronts_lv = (FrontDesc*)(d + o_fronts_lv);
  D.rows = (int32_t*)(d + o_rows);
  D.children = (int32_t*)(d + o_children);
  D.rel = (int32_t*)(d + o_rel);
  D.inv = (int32_t*)(d + o_inv);
  D.blk_dst = (int32_t*)(d + o_bdst);
  D.b_dst = (int32_t*)(d + o_rdst);
  D.level_fronts = (int32_t*)(d + o_lf);
  D.tiles = (int32_t*)(d + o_tiles);
  D.work = (WorkRec*)(d + o_work);
  D.asm_ptr = V.asm_ptr; D.asm_src = V.asm_src; D.vperm = V.vperm; D.ef = V.ef; D.et = V.et; D.off_row = V.off_row; D.off_col = V.off_col;
  D.cmask = (uint8_t*)(d + o_cmask);
  D.top_fronts = (int32_t*)(d + o_tf); D.top_children = (int32_t*)(d + o_tc); D.top_blocks = (int32_t*)(d + o_tb);
  D.top_nfronts = (int)S.top_fronts.size(); D.top_c0 = S.top_c0; D.top_ncols = 3 * S.top_nposes;
  D.top_nchild = (int)S.top_children.size(); D.top_nblk = (int)S.top_blocks.size() / 3;
  D.term = (double*)(d + o_term);
  D.Ablk = (double*)(d + o_A);
  D.bvec = (double*)(d + o_b);
  D.yvec = (double*)(d + o_y);
  D.xvec = (double*)(d + o_x);
  D.uvec = (double*)(d + o_u);
  D.Lbuf = (double*)(d + o_L);
  D.Ubuf = (double*)(d + o_U);
  launch_build_maps(ctx->stream, D, V.offbase, (const int32_t*)(d + o_rec0));
  HIP_TRY(ctx, hipGetLastError());
  D.Pan = (double*)(d + o_pan);
  D.pan_clean = false;
  D.pan_doubles = S.pan_doubles;
  D.chi2 = (double*)(d + o_chi);
  D.status = (int*)(d + o_status);
  D.ready = (int*)(d + o_ready);
  // the upper levels of the tree are solved backwards in one chained launch: as many levels as fit the workgroups that
  // are certainly resident together (the waits inside the launch cannot deadlock then); CGMR_BWD_CHAIN=0: one launch per level
  choose_bwd_chain(D, ctx->side_used ? 2 : 1, false);      // (the other half of the slots: the side stream's batches)
  choose_fwd_merge(D, ctx->side_used ? 2 : 1, false, ctx->fwd_merge_any);
  return 0;
}

// `n` extra copies of the numeric work space of the uploaded structure (the structure arrays are shared): independent
// numeric passes on the same graph -- one condensed graph per peer -- run as the jobs of one batch.  D: the first copy's view,
// copy j lies j * *stride_out bytes behind it.
int gn_replicas(cgmr_ctx* ctx, int n, GnDevice& D, size_t* stride_out) {
  const Symbolic& S = ctx->sym;
  BlobLayout N;
  size_t o_term = N.add<double>((size_t)34 * S.nE), o_A = N.add<double>((size_t)9 * (S.nf + S.nb)), o_b = N.add<double>((size_t)3 * S.nf),
         o_y = N.add<double>((size_t)3 * S.nf), o_x = N.add<double>((size_t)3 * S.nf), o_u = N.add<double>((size_t)3 * S.rows.size() + 3),
         o_L = N.add<double>((size_t)S.L_doubles + 1), o_U = N.add<double>((size_t)S.U_doubles + 1),
         o_pan = N.add<double>((size_t)S.pan_doubles + 2), o_chi = N.add<double>(8),
         o_status = N.add<int>(4), o_ready = N.add<int>(S.fronts.size() + 4), o_cmask = N.add<uint8_t>((size_t)S.nf + 16);
  const size_t per = (N.off + 255) & ~size_t(255);
  int rc = arena_reserve(ctx, ctx->rep_arena, per * (size_t)std::max(n, 1) + 256);
  if (rc) return rc;
  *stride_out = per;
  char* d = ctx->rep_arena.ptr;
  D = ctx->gn;
  D.term = (double*)(d + o_term); D.Ablk = (double*)(d + o_A); D.bvec = (double*)(d + o_b); D.yvec = (double*)(d + o_y);
  D.xvec = (double*)(d + o_x); D.uvec = (double*)(d + o_u); D.Lbuf = (double*)(d + o_L); D.Ubuf = (double*)(d + o_U); D.Pan = (double*)(d + o_pan); D.pan_clean = false;
  D.chi2 = (double*)(d + o_chi); D.status = (int*)(d + o_status); D.ready = (int*)(d + o_ready); D.cmask = (uint8_t*)(d + o_cmask);
  return 0;
}

// The analysis of (nV, ef, et) into `sym`, which holds the analysis of (prev_nV, pef, pet) when have_prev: extended from it
// where the two lists allow that, from scratch otherwise (shared by prepare_structure and the host-only test hook).
int analyze_next(Symbolic& sym, const Switches& sw, bool have_prev, int prev_nV, const std::vector<int32_t>& pef, const std::vector<int32_t>& pet, int nV,
                 int nE, const int32_t* ef, const int32_t* et, const int32_t* hub_vertices, int n_hub_vertices, const AnalyzeHooks* hooks = nullptr) {
  int n_common = 0;
  if (have_prev && nV >= prev_nV && !pef.empty()) {
    const int lim = std::min(nE, (int)pef.size());
    while (n_common < lim && pef[n_common] == ef[n_common] && pet[n_common] == et[n_common]) n_common++;
  }
  const int old_nE = (int)pef.size();
  const bool grown = n_common > 0 && (n_common == old_nE || (n_hub_vertices > 0 && 2 * n_common >= old_nE));
  if (grown) {
    Symbolic old = std::move(sym);
    return analyze(nV, nullptr, nE, ef, et, sym, sw, &old, n_common == old_nE && nE >= old_nE ? -1 : n_common, hub_vertices, n_hub_vertices, hooks);
  }
  return analyze(nV, nullptr, nE, ef, et, sym, sw, nullptr, -1, hub_vertices, n_hub_vertices, hooks);
}

// Ordering + symbolic analysis + structure upload for the edge list (ef, et), or nothing at all when the context
// still holds them for exactly this list (g2o redoes buildStructure + cs_schol on every optimize() call,
// SURVEY.md 3.2; within one key frame -- optimize(1), covariance estimate, optimize(5), graph_slam.cpp:392-393,
// 315-320 -- and within one multi-robot round the list does not change).  The analysis does not look at the fixed
// flags (they are applied numerically, prepare_pass()), so a hit is bit-identical to a miss by construction.
int prepare_structure(cgmr_ctx* ctx, int nV, int nE, const int32_t* ef, const int32_t* et, int iters, const int32_t* hub_vertices,
                      int n_hub_vertices) {
  const bool hit = ctx->sym_cache_on && ctx->sym_valid && ctx->sym_nV == nV && (int)ctx->sym_ef.size() == nE &&
                   iters <= ctx->sym_chi_cap &&
                   (nE == 0 || (memcmp(ctx->sym_ef.data(), ef, sizeof(int32_t) * nE) == 0 &&
                                memcmp(ctx->sym_et.data(), et, sizeof(int32_t) * nE) == 0));
  if (hit) {
    ctx->sym_hits++;
    ctx->sym.t_order = ctx->sym.t_struct = ctx->sym.t_upload = 0;
    return 0;
  }
  // The key-frame pattern: the cached edge list plus vertices / edges appended at the end (graph_slam.cpp:197-267 adds a
  // vertex and a few edges per key frame; a multi-robot round adds a chunk).  The ordering is then extended instead of
  // recomputed (gn_symbolic.cpp: extend_order); everything downstream of the ordering is built as for a new graph.
  // A robot's list (hub_vertices given: cgmr_graph_optimize) is its own edges, appended to, followed by the edges received
  // from the peers, replaced every round: the two lists share their front only, the rest of the new one is checked against
  // the tree edge by edge (an edge to a hub -- the gauge of a received star -- always passes).
  const bool have_prev = ctx->sym_cache_on && ctx->sym_valid;
  ctx->sym_valid = false;
  AnalyzeHooks hooks;
  int hook_rc = 0;
  hooks.blocks_ready = [&](const Symbolic& S, const int32_t* offbase) { hook_rc = gn_upload_early(ctx, S, ef, et, offbase); return hook_rc ? -100 : 0; };
  int rc = analyze_next(ctx->sym, ctx->sw, have_prev, ctx->sym_nV, ctx->sym_ef, ctx->sym_et, nV, nE, ef, et, hub_vertices, n_hub_vertices, &hooks);
  if (rc == -100) return hook_rc;                                   // (the device pass of the analysis failed: its error is set)
  if (rc == 0 && ctx->sym.extended) ctx->sym_extended++; else ctx->sym_misses++;
  if (rc) return set_err(ctx, CGMR_E_INVALID, "graph structure rejected (edge index out of range)");
  const int chi_cap = std::max(iters, 30);
  const double tu0 = wall_s();
  rc = gn_upload(ctx, ctx->sym, chi_cap);
  if (rc) return rc;
  ctx->sym.t_upload = wall_s() - tu0;
  if (ctx->sym_cache_on) {
    ctx->sym_nV = nV;
    ctx->sym_ef.assign(ef, ef + nE);
    ctx->sym_et.assign(et, et + nE);
    ctx->sym_valid = true;
  }
  ctx->sym_chi_cap = chi_cap;
  return 0;
}

// Per numeric pass: the column mask (fixed vertices; vertices whose edges are all switched off when only the
// first n_active edges take part), the status words.  ctx->vmask keeps the per-vertex flags for the caller.
int prepare_pass(cgmr_ctx* ctx, const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et, int n_active) {
  const Symbolic& S = ctx->sym;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  ctx->vmask.assign(S.nV, 0);
  if (fixed) for (int v = 0; v < S.nV; v++) ctx->vmask[v] = fixed[v] ? 1 : 0;
  if (n_active < nE) {
    std::vector<uint8_t> live(S.nV, 0);
    for (int k = 0; k < n_active; k++) { live[ef[k]] = 1; live[et[k]] = 1; }
    for (int v = 0; v < S.nV; v++) if (!live[v]) ctx->vmask[v] = 1;
  }
  HIP_TRY(ctx, hipMemsetAsync(D.status, 0, 16, st));
  if (S.nf == 0) return 0;
  int rc = pinned_mask_reserve(ctx, (size_t)S.nf);
  if (rc) return rc;
  char* pm = ctx->pinned_mask;
  for (int c = 0; c < S.nf; c++) pm[c] = (char)ctx->vmask[S.perm[c]];
  HIP_TRY(ctx, hipMemcpyAsync(D.cmask, pm, (size_t)S.nf, hipMemcpyHostToDevice, st));
  return 0;
}

// profiling mode: add up the event pairs of the launches since the last collection (call after a stream sync)
void profile_collect(cgmr_ctx* ctx) {
  for (size_t k = 0; k < ctx->ev_cls.size(); k++) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev_pool[2 * k], ctx->ev_pool[2 * k + 1]) == hipSuccess) ctx->ksec[ctx->ev_cls[k]] += 1e-3 * ms;
  }
  ctx->ev_cls.clear();
}

struct KTimer {   // optional per-launch-class timing (profiling mode only)
  cgmr_ctx* ctx;
  hipStream_t st;
  template <typename Fn>
  void run(int cls, int nlaunch, Fn&& fn) {
    if (ctx->sw.trace_launches) {                                 // debugging aid: name every launch, sync after it
      fprintf(stderr, "[cgmr] launch class %d (0 lin 1 asm 2 chi2 3 factor 4 update 5 top 6 bwd 7 poses 8 factor+update)\n", cls);
      fn();
      hipError_t e = hipStreamSynchronize(st);
      fprintf(stderr, "[cgmr]   done: %s\n", hipGetErrorString(e));
      return;
    }
    if (!ctx->profiling || st != ctx->stream || 2 * (ctx->ev_cls.size() + 1) > ctx->ev_pool.size()) { fn(); return; }
    const size_t k = ctx->ev_cls.size();
    (void)hipEventRecord(ctx->ev_pool[2 * k], ctx->stream);
    fn();
    (void)hipEventRecord(ctx->ev_pool[2 * k + 1], ctx->stream);
    ctx->ev_cls.push_back(cls);
    ctx->klaunch[cls] += nlaunch;
  }
};

void gn_pass(cgmr_ctx* ctx, double* d_poses, const GnEdges& Ed, const GnPassOpts& o) {
  gn_pass_on(ctx, ctx->gn, ctx->stream, d_poses, Ed, o);
}

void gn_pass_on(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, double* d_poses, const GnEdges& Ed, const GnPassOpts& o) {
  const bool write_l11c = o.write_l11c;
  KTimer T{ctx, st};
  T.run(0, 1, [&] { launch_linearize(st, D, d_poses, Ed, o.chi_only ? 1 : 0); });
  if (o.chi_only || D.nf == 0) {
    T.run(2, 1, [&] { launch_chi2(st, D, D.chi2 + o.chi_slot); });
    return;
  }
  // the assembled panels start from zero: H blocks and b (k_assemble), then the children's contributions level by level
  // (zeroing them for the next pass on a side stream underneath this pass's backward solve was measured slower: 5.79
  // instead of 5.47 ms per optimize(10) -- the 36 MB of writes slow the chained solve's hops more than the 8 us they hide)
  // ... but the top-block launch, one workgroup on an idle chip, clears them for the next pass with its other workgroups
  if (D.pan_doubles > 0 && !D.pan_clean) {
    if (D.njobs > 1) (void)hipMemset2DAsync(D.Pan, (size_t)D.job_stride, 0, sizeof(double) * (size_t)D.pan_doubles, (size_t)D.njobs, st);
    else (void)hipMemsetAsync(D.Pan, 0, sizeof(double) * (size_t)D.pan_doubles, st);
  }
  D.pan_clean = false;
  T.run(1, 1, [&] { launch_assemble(st, D); });                // + the chi2 sum of this iteration (slot = iterations done)
  if (Ed.typed && Ed.unary.n > 0) T.run(1, 1, [&] { launch_add_unary(st, D, Ed); });   // the priors: self edges, no assembly key
  if (o.after_assemble) o.after_assemble(st, D, o.after_assemble_arg);
  const bool trace = ctx->sw.trace_launches;
  if (trace)
    fprintf(stderr, "[cgmr] arena %p .. %p; work %p rel %p Pan %p Ablk %p bvec %p yvec %p uvec %p Lbuf %p Ubuf %p chi2 %p\n",
            (void*)ctx->gn_arena.ptr, (void*)(ctx->gn_arena.ptr + ctx->gn_arena.cap), (void*)D.work, (void*)D.rel, (void*)D.Pan,
            (void*)D.Ablk, (void*)D.bvec, (void*)D.yvec, (void*)D.uvec, (void*)D.Lbuf, (void*)D.Ubuf, (void*)D.chi2);
  for (int l = 0; l < D.nlevels; l++) {
    if (trace) {
      int maxr = 0, maxc = 0;
      for (int q = D.h_level_ptr[l]; q < D.h_level_ptr[l + 1]; q++) {
        const FrontDesc& F = ctx->sym.fronts[ctx->sym.gn_level_fronts[q]];
        maxr = std::max(maxr, 3 * F.ns);
        for (int k = 0; k < F.nchild; k++) maxc = std::max(maxc, 3 * ctx->sym.fronts[ctx->sym.children[F.child_off + k]].ns);
      }
      if (D.h_level_ptr[l + 1] - D.h_level_ptr[l] <= 2)
        for (int q = D.h_level_ptr[l]; q < D.h_level_ptr[l + 1]; q++) {
          const FrontDesc& F = ctx->sym.fronts[ctx->sym.gn_level_fronts[q]];
          fprintf(stderr, "[cgmr]   front nc %d ns %d na %d nchild %d a_cnt %d L_off %lld U_off %lld:", F.nc, F.ns, F.na, F.nchild, F.a_cnt, (long long)F.L_off, (long long)F.U_off);
          for (int k = 0; k < F.nchild; k++) { const FrontDesc& G = ctx->sym.fronts[ctx->sym.children[F.child_off + k]]; fprintf(stderr, " child(ns %d na %d U_off %lld)", G.ns, G.na, (long long)G.U_off); }
          fprintf(stderr, "\n");
        }
      fprintf(stderr, "[cgmr] level %d: %d fronts, %d work items, max r %d, max child rows %d\n", l,
              D.h_level_ptr[l + 1] - D.h_level_ptr[l], D.h_work_ptr[l + 1] - D.h_work_ptr[l], maxr, maxc);
    }
    if (l < (int)D.h_level_merge.size() && D.h_level_merge[l]) { T.run(8, 1, [&] { launch_front_level(st, D, l, write_l11c); }); continue; }
    T.run(3, 1, [&] { launch_factor_level(st, D, l, write_l11c); });
    if (D.h_tile_ptr[l + 1] > D.h_tile_ptr[l]) T.run(4, 1, [&] { launch_update_level(st, D, l); });
  }
  // the top of the tree in one launch: assembly, factorisation, forward and backward solve of the block's columns
  const bool clear_in_top = ctx->sw.clear_in_top;
  // (the chained backward solve works with L11^-1 of every front: made by the idle workgroups of the top-block launch)
  const bool chain = o.solve && D.bwd_chain_level < D.nlevels;
  if (D.top_nfronts > 0) {
    T.run(5, 1, [&] { launch_top_block(st, D, /*store_l=*/write_l11c, write_l11c, clear_in_top, chain); });
    D.pan_clean = clear_in_top && D.pan_doubles > 0;
  } else if (chain) {
    T.run(5, 1, [&] { launch_invert_fronts(st, D); });
  }
  if (!o.solve) return;
  // (the forward solve L y = b rides through k_front_factor as an extra row of every front)
  if (D.bwd_chain_level < D.nlevels) T.run(6, 1, [&] { launch_bwd_chain(st, D); });
  for (int l = D.bwd_chain_level - 1; l >= 0; l--) T.run(6, 1, [&] { launch_bwd_level(st, D, l); });
  if (o.update_poses)
    T.run(7, 1, [&] { if (Ed.chordal_stage == kChordalRotation) launch_apply_rotation(st, D, d_poses); else launch_update(st, D, d_poses); });
}

int LevelwiseScope::arm(hipStream_t st, int it0) {
  count_timeout(ctx);
  armed = true;
  chain_was = D.bwd_chain_level;
  merge_was = D.h_level_merge;
  D.bwd_chain_level = D.nlevels;
  D.h_level_merge.assign(D.nlevels, 0);
  const int fresh[4] = {0, it0, 0, 0};
  HIP_TRY(ctx, hipMemcpyAsync(D.status, fresh, sizeof fresh, hipMemcpyHostToDevice, st));
  return 0;
}

// What an optimisation call does around its device work, whatever the algorithm: the structure and the masks with their
// wall-clock marks, the timing events, the caller's host copy of the estimates, the wait, cgmr_gn_timing's five entries.
struct GnCall {
  cgmr_ctx* ctx;
  int nV;
  double* d_poses;
  double t0, t1 = 0, t2 = 0;
  double* poses_host = nullptr;
  struct Readback { void* dst; const void* src; size_t bytes; };

  GnCall(cgmr_ctx* c, int nv, double* dp) : ctx(c), nV(nv), d_poses(dp), t0(wall_s()) {}
  // chi_slots: iterations whose chi2 slot the structure's work space must hold
  int prepare(const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et, int n_active, int chi_slots,
              const int32_t* hub_vertices, int n_hub_vertices) {
    int rc = prepare_structure(ctx, nV, nE, ef, et, chi_slots, hub_vertices, n_hub_vertices);
    if (rc) return rc;
    t1 = wall_s();
    rc = prepare_pass(ctx, fixed, nE, ef, et, n_active);
    t2 = wall_s();
    return rc;
  }
  // the device work starts here (ev0; its end: the last hipEventRecord of ev1 before a wait)
  int begin() {
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    // the caller's host copy of the estimates rides in every wait (a robot graph whose peers have asked for condensed graphs
    // picks their gauges from it right after the solve)
    poses_host = ctx->poses_out_host;
    ctx->poses_out_host = nullptr;
    return 0;
  }
  int wait(std::initializer_list<Readback> what) {
    hipStream_t st = ctx->stream;
    for (const Readback& r : what)
      if (r.bytes) HIP_TRY(ctx, hipMemcpyAsync(r.dst, r.src, r.bytes, hipMemcpyDeviceToHost, st));
    if (poses_host && nV > 0) HIP_TRY(ctx, hipMemcpyAsync(poses_host, d_poses, 24 * (size_t)nV, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipGetLastError());
    return 0;
  }
  void finish() {
    const Symbolic& S = ctx->sym;
    if (ctx->profiling) profile_collect(ctx);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->timing[0] = S.t_order;
    ctx->timing[1] = S.t_struct;
    ctx->timing[2] = (t2 - t1) + S.t_upload;     // structure blob (host staging + H2D enqueue) + per-pass masks
    ctx->timing[3] = 1e-3 * ms;
    ctx->timing[4] = wall_s() - t0;
  }
};

int gn_run(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* ef,
           const int32_t* et, const GnEdges& Ed, int iters, double* chi2_out, const int32_t* hub_vertices, int n_hub_vertices) {
  GnCall call(ctx, nV, d_poses);
  int rc = call.prepare(fixed, nE, ef, et, Ed.n_active, iters, hub_vertices, n_hub_vertices);
  if (rc) return rc;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  // (robust statistics: written by the final chi-only pass, at the estimate the call returns)
  GnEdges Ei = Ed;
  Ei.rk.stats = nullptr;
  Ei.mx.sel_out = nullptr;                 // (a mixture's selection: written by the same pass)
  // iterations it0 .. iters - 1, then the chi-only pass at the estimate they leave
  auto queue_from = [&](int it0) {
    GnPassOpts o;
    for (o.chi_slot = it0; o.chi_slot < iters; o.chi_slot++) gn_pass(ctx, d_poses, Ei, o);
    o.chi_only = true;
    gn_pass(ctx, d_poses, Ed, o);
  };
  rc = call.begin();
  if (rc) return rc;
  // Every launch of a GN iteration is the same whatever the iteration's number (status[1] on the device supplies the
  // chi2 slot and the failure tag): CGMR_GRAPH=1 captures one iteration into a hipGraph and replays it.
  const bool graph_mode = ctx->sw.graph, trace_launches = ctx->sw.trace_launches;
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  if (graph_mode && !ctx->profiling && !trace_launches && iters >= 2 && st != nullptr && D.nf > 0 && !Ed.mix) {
    gn_init_kernels();
    HIP_TRY(ctx, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    gn_pass(ctx, d_poses, Ei, GnPassOpts());
    HIP_TRY(ctx, hipStreamEndCapture(st, &graph));
    HIP_TRY(ctx, hipGraphInstantiate(&graph_exec, graph, nullptr, nullptr, 0));
    for (int it = 0; it < iters; it++) HIP_TRY(ctx, hipGraphLaunch(graph_exec, st));
    queue_from(iters);
  } else {
    queue_from(0);
  }
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, st));
  const double t3 = wall_s();
  std::vector<double> chi(iters + 1);
  int status4[4] = {0, 0, 0, 0};
  const std::initializer_list<GnCall::Readback> results = {{chi.data(), D.chi2, sizeof(double) * (iters + 1)}, {status4, D.status, sizeof status4}};
  rc = call.wait(results);
  if (rc) return rc;
  {
    // CGMR_GN_TRACE: where a solve's wall time goes beside the analysis -- queueing the launches, waiting for the stream
    if (ctx->sw.gn_trace) {
      const double t4 = wall_s();
      ctx->trace_n++; ctx->trace_sum[0] += call.t1 - call.t0; ctx->trace_sum[1] += call.t2 - call.t1; ctx->trace_sum[2] += t3 - call.t2; ctx->trace_sum[3] += t4 - t3;
    }
  }
  if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
  if (graph) (void)hipGraphDestroy(graph);
  if (status4[2] != 0 && status4[0] > 0) {
    // A bounded wait of the chained backward solve ran out.  The iteration it happened in (status[0] - 1) and the later ones
    // were not applied (k_update_poses leaves the poses alone once status[0] is set), so they are repeated from the poses as
    // they stand, level-wise, and the call goes on as if nothing had happened.
    const int it0 = status4[0] - 1;
    LevelwiseScope levelwise(ctx, D);
    rc = levelwise.arm(st, it0);
    if (rc) return rc;
    queue_from(it0);
    rc = call.wait(results);
    if (rc) return rc;
    if (status4[2] != 0) return set_err(ctx, CGMR_E_TIMEOUT, "backward solve: a bounded device-side wait ran out twice");
  }
  const int status = status4[0];
  call.finish();
  if (chi2_out) memcpy(chi2_out, chi.data(), sizeof(double) * (iters + 1));
  if (status != 0)
    return set_err(ctx, CGMR_E_CHOLESKY_BASE - (status - 1),
                   "Cholesky failed (non-positive pivot) in GN iteration %d; poses left at the last good update",
                   status - 1);
  return CGMR_OK;
}

// Chordal initialisation (include/cgmr.h: cgmr_chordal_initialize; init_kernels.hip): one structure, then one pass per
// requested stage -- the stage's mask, gn_pass with the stage in GnEdges -- between two chi-only passes of the ordinary
// linearisation, and one wait.  in_rot / in_tr [nV]: the vertices some term of the stage touches; the others are left out of it
// through its mask like the fixed ones.  The chi2 slots: pass p's own cost in slot p (k_assemble, from status[1]), the SE(2)
// chi2 at the start and at the result in slots 4 and 5.  A non-positive pivot in pass p: status[0] = p + 1, that pass and the
// later ones change nothing (k_apply_rotation and k_update_poses skip), the call returns GN's code for iteration p.
int chordal_run(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et,
                const GnEdges& Ed, int stages, const uint8_t* in_rot, const uint8_t* in_tr, double* chi2_out, int32_t* counts_out) {
  constexpr int kSlotStart = 4, kSlotEnd = 5, kSlots = 6;
  GnCall call(ctx, nV, d_poses);
  int rc = prepare_structure(ctx, nV, nE, ef, et, kSlots);
  if (rc) return rc;
  call.t1 = wall_s();
  const Symbolic& S = ctx->sym;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  int seq[2], npass = 0;
  if (stages & kChordalRotation) seq[npass++] = kChordalRotation;
  if (stages & kChordalTranslation) seq[npass++] = kChordalTranslation;
  // the passes' column masks, side by side in pinned memory: they stay as they are until the call's last wait
  rc = pinned_mask_reserve(ctx, (size_t)2 * S.nf + 1);
  if (rc) return rc;
  int solved[2] = {0, 0};
  for (int p = 0; p < npass; p++) {
    const uint8_t* in = seq[p] == kChordalRotation ? in_rot : in_tr;
    ctx->vmask.assign(S.nV, 0);
    for (int v = 0; v < S.nV; v++) ctx->vmask[v] = (fixed[v] || !in[v]) ? 1 : 0;
    char* pm = ctx->pinned_mask + (size_t)p * S.nf;
    for (int c = 0; c < S.nf; c++) {
      pm[c] = (char)ctx->vmask[S.perm[c]];
      solved[p] += pm[c] ? 0 : 1;
    }
  }
  HIP_TRY(ctx, hipMemsetAsync(D.status, 0, 16, st));
  call.t2 = wall_s();
  bool queue_failed = false;
  // the passes p0 .. npass - 1, then the chi-only pass at the estimate they leave
  auto queue_from = [&](int p0) {
    GnPassOpts o;
    for (int p = p0; p < npass; p++) {
      if (S.nf > 0 && hipMemcpyAsync(D.cmask, ctx->pinned_mask + (size_t)p * S.nf, (size_t)S.nf, hipMemcpyHostToDevice, st) != hipSuccess) queue_failed = true;
      GnEdges Es = Ed;
      Es.chordal_stage = seq[p];
      o.chi_slot = p;
      gn_pass(ctx, d_poses, Es, o);
    }
    o.chi_only = true;
    o.chi_slot = kSlotEnd;
    gn_pass(ctx, d_poses, Ed, o);
  };
  rc = call.begin();
  if (rc) return rc;
  {
    GnPassOpts o;
    o.chi_only = true;
    o.chi_slot = kSlotStart;
    gn_pass(ctx, d_poses, Ed, o);
  }
  queue_from(0);
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, st));
  double chi[kSlots] = {0, 0, 0, 0, 0, 0};
  int status4[4] = {0, 0, 0, 0};
  const std::initializer_list<GnCall::Readback> results = {{chi, D.chi2, sizeof chi}, {status4, D.status, sizeof status4}};
  rc = call.wait(results);
  if (rc) return rc;
  int degenerate_kept = 0;
  if (status4[2] != 0 && status4[0] > 0) {
    // A bounded wait of the chained backward solve ran out in pass status[0] - 1: that pass and the later ones were not applied
    // and are repeated level-wise (gn_run).  The fresh status words drop the count of an earlier rotation pass: kept here.
    const int p0 = std::min(status4[0] - 1, npass - 1);
    if (p0 > 0) degenerate_kept = status4[kChordalDegenerateWord];
    LevelwiseScope levelwise(ctx, D);
    rc = levelwise.arm(st, p0);
    if (rc) return rc;
    queue_from(p0);
    rc = call.wait(results);
    if (rc) return rc;
    if (status4[2] != 0) return set_err(ctx, CGMR_E_TIMEOUT, "backward solve: a bounded device-side wait ran out twice");
  }
  if (queue_failed) return set_err(ctx, CGMR_E_HIP, "cgmr_chordal_initialize: a stage's mask could not be queued");
  const int status = status4[0];
  call.finish();
  if (chi2_out) { chi2_out[0] = chi[kSlotStart]; chi2_out[1] = chi[kSlotEnd]; }
  if (counts_out) {
    counts_out[0] = counts_out[1] = 0;
    for (int p = 0; p < npass; p++)
      if (status == 0 || p < status - 1) counts_out[seq[p] == kChordalRotation ? 0 : 1] = solved[p];
    counts_out[2] = status4[kChordalDegenerateWord] + degenerate_kept;
  }
  if (status != 0)
    return set_err(ctx, CGMR_E_CHOLESKY_BASE - (status - 1),
                   "Cholesky failed (non-positive pivot) in the %s stage of the chordal initialisation; poses left as they were before it",
                   seq[std::min(status - 1, npass - 1)] == kChordalRotation ? "rotation" : "translation");
  return CGMR_OK;
}

// Levenberg-Marquardt and dogleg are two policies of one driver.  A policy P supplies
//   State, L (its device buffers; L.S the state, L.saved the saved poses), kName;
//   reserve():      its arena laid out as state | records | work space, L bound to it; the bytes of state + records
//   start():        the state a call begins with;
//   queue_round():  the launches of one round, from the host's copy of the state;
//   also_read():    what a round's wait reads back beside state + records;
//   empty_system(): the closed-form answer when nothing can move, into the host's copy of state + records;
//   finish():       records and statistics out, the call's return code;
//   kRunsEmpty:     its rounds also serve a system with nothing to move (else: empty_system()).
// The driver owns the rest: upload, the saved poses, the rounds with their one wait each, a timed-out round's repeat
// (LevelwiseScope), the final pass of the robust statistics.
template <typename P>
static int tr_run(cgmr_ctx* ctx, P& pol, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et,
                  const GnEdges& Ed, int iters, const int32_t* hub_vertices, int n_hub_vertices) {
  GnCall call(ctx, nV, d_poses);
  // (the chi2 slots a trial uses: slot 0 only -- the cache entry of a Gauss-Newton call on the same edge list serves)
  int rc = call.prepare(fixed, nE, ef, et, Ed.n_active, 1, hub_vertices, n_hub_vertices);
  if (rc) return rc;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  size_t rec_bytes = 0;
  rc = pol.reserve(ctx, iters, nV, D.nf, nE, &rec_bytes);
  if (rc) return rc;
  char* const d = (char*)pol.L.S;
  std::vector<char> h(rec_bytes, 0);                          // the host's copy of state + records
  typename P::State hs = pol.start(iters);
  memcpy(h.data(), &hs, sizeof hs);
  HIP_TRY(ctx, hipMemcpyAsync(d, h.data(), rec_bytes, hipMemcpyHostToDevice, st));
  if (nV > 0) HIP_TRY(ctx, hipMemcpyAsync(pol.L.saved, d_poses, 24 * (size_t)nV, hipMemcpyDeviceToDevice, st));
  rc = call.begin();
  if (rc) return rc;
  int64_t waits = 0;
  if ((D.nf == 0 || iters == 0) && !P::kRunsEmpty) {
    // nothing to move (or nothing asked): chi2 at x, and what g2o makes of an empty system
    GnPassOpts chi_pass;
    chi_pass.chi_only = true;
    gn_pass(ctx, d_poses, Ed, chi_pass);
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, st));
    double chi0 = 0;
    rc = call.wait({{&chi0, D.chi2, sizeof(double)}});
    if (rc) return rc;
    waits = 1;
    pol.empty_system(hs, h.data(), chi0, iters);
  } else {
    LevelwiseScope levelwise(ctx, D);
    GnEdges Ei = Ed;                                         // (robust statistics: one chi-only pass on the final poses below)
    Ei.rk.stats = nullptr;
    Ei.mx.sel_out = nullptr;                                    // (a mixture's selection: the same pass)
    for (;;) {
      pol.queue_round(ctx, D, st, nV, d_poses, Ei, hs, iters);
      HIP_TRY(ctx, hipEventRecord(ctx->ev1, st));
      rc = call.wait({{h.data(), d, rec_bytes}, pol.also_read(D)});
      if (rc) return rc;
      waits++;
      memcpy(&hs, h.data(), sizeof hs);
      if (hs.halted) {
        // A bounded wait ran out in a pass (status[2]): not a numerical verdict.  The poses are those the trial started from
        // and nothing queued behind it changed anything; the call goes on from the state as it stands, level-wise.
        if (levelwise.armed) return set_err(ctx, CGMR_E_TIMEOUT, "%s: a bounded device-side wait ran out twice", P::kName);
        rc = levelwise.arm(st);
        if (rc) return rc;
        hs.halted = 0;
        hs.accept = -1;
        HIP_TRY(ctx, hipMemcpyAsync(pol.L.S, &hs, sizeof hs, hipMemcpyHostToDevice, st));
        continue;
      }
      if (hs.done) break;
    }
    if (Ed.rk.stats || Ed.mx.sel_out) launch_linearize(st, D, d_poses, Ed, 1);   // (read back by the caller, behind the stream)
  }
  call.finish();
  return pol.finish(ctx, hs, h.data(), std::min(hs.iter, iters), iters, waits);
}

// records [0, ran) of an iteration's array to the caller's (nullable), zeros behind them
template <typename T>
static void records_out(T* out, const T* rec, int ran, int iters) {
  if (out) for (int k = 0; k < iters; k++) out[k] = k < ran ? rec[k] : T(0);
}
static void chi2_records_out(double* out, const double* rec, int ran, int iters) {
  if (out) for (int k = 0; k <= iters; k++) out[k] = rec[std::min(k, ran)];
}

// g2o's OptimizationAlgorithmLevenberg defaults [g2o-recalled]
static cgmr_lm_params lm_defaults() {
  cgmr_lm_params p;
  p.tau = 1e-5; p.initial_lambda = -1; p.max_trials = 10; p.good_step_lower = 1.0 / 3; p.good_step_upper = 2.0 / 3;
  return p;
}

struct LmPolicy {
  using State = LmState;
  static constexpr const char* kName = "Levenberg-Marquardt";
  static constexpr bool kRunsEmpty = false;
  cgmr_lm_params P;
  double *chi2_out, *lambda_out;
  int32_t *trials_out, *iters_done;
  LmDev L;
  size_t o_chi = 0, o_lam = 0, o_tri = 0;
  int status4[4] = {0, 0, 0, 0};

  // lm arena: state | chi2 records [iters + 1] | lambda records [iters] | trial records [iters] | saved poses [3 nV]
  int reserve(cgmr_ctx* ctx, int iters, int nV, int, int, size_t* rec_bytes) {
    BlobLayout B;
    B.add<LmState>(1);
    o_chi = B.add<double>((size_t)iters + 1); o_lam = B.add<double>((size_t)iters + 1); o_tri = B.add<int32_t>((size_t)iters + 1);
    *rec_bytes = B.off;
    const size_t o_saved = B.add<double>(3 * (size_t)std::max(nV, 1));
    int rc = arena_reserve(ctx, ctx->lm_arena, B.off + 256);
    if (rc) return rc;
    char* d = ctx->lm_arena.ptr;
    L.S = (LmState*)d; L.rec_chi = (double*)(d + o_chi); L.rec_lambda = (double*)(d + o_lam);
    L.rec_trials = (int32_t*)(d + o_tri); L.saved = (double*)(d + o_saved);
    return 0;
  }
  LmState start(int iters) const {
    LmState hs;
    hs.tau = P.tau; hs.initial_lambda = P.initial_lambda; hs.max_trials = P.max_trials;
    hs.lower = P.good_step_lower; hs.upper = P.good_step_upper; hs.iters = iters;
    return hs;
  }
  static void damp(hipStream_t st, const GnDevice& D, void* self) { launch_lm_damp(st, D, ((LmPolicy*)self)->L.S); }
  static void init_and_damp(hipStream_t st, const GnDevice& D, void* self) {
    launch_lm_init(st, D, ((LmPolicy*)self)->L.S);
    damp(st, D, self);
  }
  // One trial, the same launches whatever happens (lm_kernels.hip): linearise + assemble + damp + factor + solve + update at x,
  // chi-only linearise at x', the verdict, then restore x or keep x'.
  void trial(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, int nV, double* d_poses, const GnEdges& Ed, bool init) {
    GnPassOpts o;
    o.after_assemble = init ? init_and_damp : damp;
    o.after_assemble_arg = this;
    gn_pass_on(ctx, D, st, d_poses, Ed, o);
    launch_linearize(st, D, d_poses, Ed, 1);
    launch_lm_decide(st, D, L);
    launch_tr_commit(st, nV, d_poses, L.saved, &L.S->accept);
  }
  // one trial per iteration still to run; a rejected trial leaves its iteration to the next round
  void queue_round(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, int nV, double* d_poses, const GnEdges& Ed, const LmState& hs, int iters) {
    const int n_trials = iters - hs.iter;
    for (int t = 0; t < n_trials; t++) trial(ctx, D, st, nV, d_poses, Ed, t == 0);   // (k_lm_init: a no-op once lambda is set)
  }
  GnCall::Readback also_read(const GnDevice& D) { return {status4, D.status, sizeof status4}; }
  // with iterations asked, the first trial's step is zero, rho = 0: g2o terminates after it, lambda grown once by nu
  void empty_system(LmState& hs, char* h, double chi0, int iters) const {
    hs.iter = iters > 0 ? 1 : 0;
    hs.lambda = 2 * (P.initial_lambda > 0 ? P.initial_lambda : 0.0);
    hs.total_trials = hs.iter;
    double* rc_chi = (double*)(h + o_chi);
    rc_chi[0] = chi0;
    if (hs.iter) { rc_chi[1] = chi0; ((double*)(h + o_lam))[0] = hs.lambda; ((int32_t*)(h + o_tri))[0] = 1; }
  }
  int finish(cgmr_ctx* ctx, const LmState& hs, const char* h, int ran, int iters, int64_t waits) const {
    chi2_records_out(chi2_out, (const double*)(h + o_chi), ran, iters);
    records_out(lambda_out, (const double*)(h + o_lam), ran, iters);
    records_out(trials_out, (const int32_t*)(h + o_tri), ran, iters);
    if (iters_done) *iters_done = ran;
    ctx->lm_stats[0] = waits;
    ctx->lm_stats[1] = hs.total_trials;
    return CGMR_OK;
  }
};

int lm_run(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et,
           const GnEdges& Ed, int iters, const cgmr_lm_params* params, double* chi2_out, double* lambda_out, int32_t* trials_out,
           int32_t* iters_done, const int32_t* hub_vertices, int n_hub_vertices) {
  const cgmr_lm_params P = params ? *params : lm_defaults();
  if (!(P.max_trials >= 1) || !(P.tau >= 0) || !(P.good_step_lower > 0) || !(P.good_step_upper > 0) || !std::isfinite(P.tau) ||
      !std::isfinite(P.initial_lambda) || !std::isfinite(P.good_step_lower) || !std::isfinite(P.good_step_upper))
    return set_err(ctx, CGMR_E_INVALID, "cgmr_lm_optimize: max_trials must be >= 1, tau >= 0, the step scales > 0, all finite");
  LmPolicy pol{P, chi2_out, lambda_out, trials_out, iters_done};
  return tr_run(ctx, pol, nV, d_poses, fixed, nE, ef, et, Ed, iters, hub_vertices, n_hub_vertices);
}

// g2o's OptimizationAlgorithmDogleg defaults [g2o-recalled]
static cgmr_dl_params dl_defaults() {
  cgmr_dl_params p;
  p.initial_delta = 1e4; p.max_trials = 100; p.initial_lambda = 1e-7; p.lambda_factor = 10;
  return p;
}

static bool dl_params_valid(const cgmr_dl_params& P) {
  return P.max_trials >= 1 && std::isfinite(P.initial_delta) && P.initial_delta > 0 && std::isfinite(P.initial_lambda) &&
         P.initial_lambda > 0 && std::isfinite(P.lambda_factor) && P.lambda_factor > 1;
}

bool dl_params_ok(const cgmr_dl_params* p) { return !p || dl_params_valid(*p); }

struct DlPolicy {
  using State = DlState;
  static constexpr const char* kName = "dogleg";
  static constexpr bool kRunsEmpty = false;
  cgmr_dl_params P;
  double *chi2_out, *delta_out;
  int32_t *trials_out, *step_out, *iters_done;
  DlDev L;
  size_t o_chi = 0, o_del = 0, o_tri = 0, o_stp = 0;
  int n_cont = 1;                                            // tails the last round gave an open iteration

  // dl arena: state | chi2 [iters + 1] | delta, trials, steps [iters] | saved poses [3 nV] | hgn, hsd [3 nf] | quad partials
  int reserve(cgmr_ctx* ctx, int iters, int nV, int nf, int nE, size_t* rec_bytes) {
    BlobLayout B;
    B.add<DlState>(1);
    o_chi = B.add<double>((size_t)iters + 1); o_del = B.add<double>((size_t)iters + 1);
    o_tri = B.add<int32_t>((size_t)iters + 1); o_stp = B.add<int32_t>((size_t)iters + 1);
    *rec_bytes = B.off;
    const size_t nf3 = 3 * (size_t)std::max(nf, 1);
    const size_t o_saved = B.add<double>(3 * (size_t)std::max(nV, 1)), o_hgn = B.add<double>(nf3), o_hsd = B.add<double>(nf3),
                 o_q = B.add<double>((size_t)std::max((nE + 255) / 256, 1));
    int rc = arena_reserve(ctx, ctx->dl_arena, B.off + 256);
    if (rc) return rc;
    char* d = ctx->dl_arena.ptr;
    L.S = (DlState*)d; L.rec_chi = (double*)(d + o_chi); L.rec_delta = (double*)(d + o_del);
    L.rec_trials = (int32_t*)(d + o_tri); L.rec_step = (int32_t*)(d + o_stp); L.saved = (double*)(d + o_saved);
    L.hgn = (double*)(d + o_hgn); L.hsd = (double*)(d + o_hsd); L.qpart = (double*)(d + o_q);
    return 0;
  }
  DlState start(int iters) const {
    DlState hs;
    hs.delta = P.initial_delta; hs.lambda = P.initial_lambda; hs.lambda_factor = P.lambda_factor; hs.max_trials = P.max_trials;
    hs.iters = iters;
    return hs;
  }
  static void damp(hipStream_t st, const GnDevice& D, void* self) { launch_dl_damp(st, D, ((DlPolicy*)self)->L.S); }
  // A head (dl_kernels.hip): linearise + assemble + [damp] + factor + solve at x (the step is left to the tails), b^T H b,
  // k_dl_begin.
  void head(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, double* d_poses, const GnEdges& Ed) {
    GnPassOpts o;
    o.update_poses = false;
    o.after_assemble = damp;
    o.after_assemble_arg = this;
    gn_pass_on(ctx, D, st, d_poses, Ed, o);
    launch_dl_quad(st, D, D.bvec, L.qpart);
    launch_dl_begin(st, D, L);
  }
  // A tail: the step for the current delta, h^T H h, update, chi-only linearise at x (+) h, the verdict, keep or restore x.
  void tail(GnDevice& D, hipStream_t st, int nV, double* d_poses, const GnEdges& Ed) {
    launch_dl_step(st, D, L);
    launch_dl_quad(st, D, D.xvec, L.qpart);
    launch_update(st, D, d_poses);
    launch_linearize(st, D, d_poses, Ed, 1);
    launch_dl_decide(st, D, L);
    launch_tr_commit(st, nV, d_poses, L.saved, &L.S->accept);
  }
  // an open iteration (its GN step solved, no good step yet) gets tails only, doubling in number from round to round; every
  // iteration not started yet gets a head and a tail
  void queue_round(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, int nV, double* d_poses, const GnEdges& Ed, const DlState& hs, int iters) {
    const bool open = hs.solved != 0;
    if (open) {
      n_cont = std::min(2 * n_cont, P.max_trials - hs.trial);
      for (int t = 0; t < n_cont; t++) tail(D, st, nV, d_poses, Ed);
    }
    const int n_new = iters - hs.iter - (open ? 1 : 0);
    for (int t = 0; t < n_new; t++) {
      head(ctx, D, st, d_poses, Ed);
      tail(D, st, nV, d_poses, Ed);
    }
  }
  GnCall::Readback also_read(const GnDevice&) { return {nullptr, nullptr, 0}; }
  // with iterations asked, g2o's empty system gives h = 0 and rho = 0 on every trial: one iteration of max_trials GN trials,
  // delta halved on each, Terminate
  void empty_system(DlState& hs, char* h, double chi0, int iters) const {
    double* rc_chi = (double*)(h + o_chi);
    rc_chi[0] = chi0;
    if (iters == 0) return;
    for (int q = 0; q < P.max_trials; q++) hs.delta *= 0.5;
    hs.iter = 1;
    hs.total_trials = P.max_trials;
    hs.terminated = 1;
    rc_chi[1] = chi0;
    ((double*)(h + o_del))[0] = hs.delta;
    ((int32_t*)(h + o_tri))[0] = P.max_trials;
    ((int32_t*)(h + o_stp))[0] = CGMR_DL_STEP_GN;
  }
  int finish(cgmr_ctx* ctx, const DlState& hs, const char* h, int ran, int iters, int64_t waits) const {
    chi2_records_out(chi2_out, (const double*)(h + o_chi), ran, iters);
    records_out(delta_out, (const double*)(h + o_del), ran, iters);
    records_out(trials_out, (const int32_t*)(h + o_tri), ran, iters);
    records_out(step_out, (const int32_t*)(h + o_stp), ran, iters);
    if (iters_done) *iters_done = ran;
    ctx->dl_stats[0] = waits;
    ctx->dl_stats[1] = hs.total_trials;
    ctx->dl_stats[2] = hs.factorisations;
    if (hs.failed)
      return set_err(ctx, CGMR_E_CHOLESKY_BASE - ran,
                     "dogleg: H + currentLambda I not positive definite with currentLambda at 1e3 in iteration %d (g2o's Fail); "
                     "poses left at the last accepted step", ran);
    return CGMR_OK;
  }
};

int dl_run(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et,
           const GnEdges& Ed, int iters, const cgmr_dl_params* params, double* chi2_out, double* delta_out, int32_t* trials_out,
           int32_t* step_out, int32_t* iters_done, const int32_t* hub_vertices, int n_hub_vertices) {
  const cgmr_dl_params P = params ? *params : dl_defaults();
  if (!dl_params_valid(P))
    return set_err(ctx, CGMR_E_INVALID,
                   "cgmr_dl_optimize: max_trials must be >= 1, initial_delta / initial_lambda > 0, lambda_factor > 1, all finite");
  DlPolicy pol{P, chi2_out, delta_out, trials_out, step_out, iters_done};
  return tr_run(ctx, pol, nV, d_poses, fixed, nE, ef, et, Ed, iters, hub_vertices, n_hub_vertices);
}

// SparseOptimizer::computeInitialGuess with unit edge cost [g2o-recalled]: breadth-first from the fixed
// vertices over the given edges (edge order breaks ties), x_to = x_from * z or x_from = x_to * z^-1.
void initial_guess_host(int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et,
                        const double* meas) {
  auto norm = [](double t) {
    const double pi = 3.14159265358979323846;
    if (t >= -pi && t < pi) return t;
    return t - 2 * pi * std::floor((t + pi) / (2 * pi));
  };
  std::vector<int> deg(nV + 1, 0);
  for (int k = 0; k < nE; k++) { deg[ef[k] + 1]++; deg[et[k] + 1]++; }
  for (int v = 0; v < nV; v++) deg[v + 1] += deg[v];
  std::vector<int> inc(2 * (size_t)nE + 1), pos(deg.begin(), deg.end() - 1);
  for (int k = 0; k < nE; k++) { inc[pos[ef[k]]++] = k; inc[pos[et[k]]++] = k; }
  std::vector<uint8_t> seen(nV, 0);
  std::vector<int> queue;
  queue.reserve(nV);
  for (int v = 0; v < nV; v++) if (fixed[v] && deg[v + 1] > deg[v]) { seen[v] = 1; queue.push_back(v); }
  for (size_t qh = 0; qh < queue.size(); qh++) {
    int u = queue[qh];
    for (int p = deg[u]; p < deg[u + 1]; p++) {
      int k = inc[p];
      int w = (ef[k] == u) ? et[k] : ef[k];
      if (seen[w]) continue;
      seen[w] = 1;
      const double* a = poses + 3 * (size_t)u;
      double z[3] = {meas[3 * k], meas[3 * k + 1], meas[3 * k + 2]};
      if (ef[k] != u) {   // z^-1
        double c = std::cos(z[2]), s = std::sin(z[2]);
        double ix = -(c * z[0] + s * z[1]), iy = -(-s * z[0] + c * z[1]);
        z[0] = ix; z[1] = iy; z[2] = -z[2];
      }
      double c = std::cos(a[2]), s = std::sin(a[2]);
      double* o = poses + 3 * (size_t)w;
      o[0] = a[0] + c * z[0] - s * z[1];
      o[1] = a[1] + s * z[0] + c * z[1];
      o[2] = norm(a[2] + z[2]);
      queue.push_back(w);
    }
  }
}

// The robust description of an entry point (include/cgmr.h: cgmr_robust) into Ed, checked before anything is queued.  The host
// entry points' kind / delta arrays are staged through rk_arena; the device ones are read back once to be checked.  The
// statistics (2 nE doubles: e2, then rho1) land in rk_arena behind them.  rk == nullptr: nothing (the plain call).
static int robust_setup(cgmr_ctx* ctx, const cgmr_robust* rk, int nE, bool dev, GnEdges& Ed, const char* who) {
  if (!rk) return 0;
  const size_t n = (size_t)std::max(nE, 0);
  std::vector<uint8_t> hk;
  std::vector<double> hd;
  const uint8_t* ck = rk->kind;
  const double* cd = rk->delta;
  if (dev && n > 0 && (rk->kind || rk->delta)) {
    if (rk->kind) { hk.resize(n); HIP_TRY(ctx, hipMemcpyAsync(hk.data(), rk->kind, n, hipMemcpyDeviceToHost, ctx->stream)); ck = hk.data(); }
    if (rk->delta) { hd.resize(n); HIP_TRY(ctx, hipMemcpyAsync(hd.data(), rk->delta, 8 * n, hipMemcpyDeviceToHost, ctx->stream)); cd = hd.data(); }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  bool ok = rk->default_kind >= CGMR_RK_NONE && rk->default_kind <= CGMR_RK_DCS;
  if (ok && !rk->kind && !rk->delta) ok = robust_valid(rk->default_kind, rk->default_delta);
  for (size_t k = 0; ok && k < n && (ck || cd); k++)
    ok = robust_valid(ck ? ck[k] : rk->default_kind, cd ? cd[k] : rk->default_delta);
  if (!ok)
    return set_err(ctx, CGMR_E_INVALID, "%s: a robust kernel kind must be 0..7, its delta finite and > 0 (kind 0 excepted)", who);
  const bool stats = n > 0 && (rk->edge_chi2_out || rk->weight_out);
  const size_t ok_ = 0, od = (n + 255) & ~size_t(255), os = od + ((8 * n + 255) & ~size_t(255));
  if (stats || (!dev && (rk->kind || rk->delta))) {
    int rc = arena_reserve(ctx, ctx->rk_arena, os + 16 * n + 256);
    if (rc) return rc;
  }
  char* d = ctx->rk_arena.ptr;
  Ed.robust = true;
  Ed.rk.kind0 = rk->default_kind; Ed.rk.delta0 = rk->default_delta;
  if (dev) { Ed.rk.kind = rk->kind; Ed.rk.delta = rk->delta; }
  else {
    if (rk->kind && n > 0) { HIP_TRY(ctx, hipMemcpyAsync(d + ok_, rk->kind, n, hipMemcpyHostToDevice, ctx->stream)); Ed.rk.kind = (const uint8_t*)(d + ok_); }
    if (rk->delta && n > 0) { HIP_TRY(ctx, hipMemcpyAsync(d + od, rk->delta, 8 * n, hipMemcpyHostToDevice, ctx->stream)); Ed.rk.delta = (const double*)(d + od); }
  }
  Ed.rk.stats = stats ? (double*)(d + os) : nullptr;
  return 0;
}

// the statistics of the call's final pass to the caller's host arrays
static int robust_stats_out(cgmr_ctx* ctx, const cgmr_robust* rk, int nE, const GnEdges& Ed) {
  if (!rk || !Ed.rk.stats) return 0;
  if (rk->edge_chi2_out) HIP_TRY(ctx, hipMemcpyAsync(rk->edge_chi2_out, Ed.rk.stats, 8 * (size_t)nE, hipMemcpyDeviceToHost, ctx->stream));
  if (rk->weight_out) HIP_TRY(ctx, hipMemcpyAsync(rk->weight_out, Ed.rk.stats + nE, 8 * (size_t)nE, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

// The factor types of a typed entry point (include/cgmr.h: cgmr_factor_types), checked on the host before the device is
// touched: every vertex kind 0 or 1, every edge kind with the vertex kinds and the arity its factor needs.  `any`: some kind
// is not zero (all zero: the call is the plain one, bit for bit -- the plain launches).  The priors grouped by vertex, in edge
// order, for k_add_unary.
struct TypedHost {
  bool any = false;
  std::vector<uint8_t> vk, ek;
  std::vector<int32_t> uv_vertex, uv_ptr, uv_edge;
};
static int typed_check(cgmr_ctx* ctx, const char* who, const cgmr_factor_types* ft, int nV, int nE, const int32_t* ef, const int32_t* et,
                       TypedHost& T) {
  if (!ft) return 0;                                          // (the plain call: nothing is built)
  T.vk.assign((size_t)std::max(nV, 0), 0);
  T.ek.assign((size_t)std::max(nE, 0), 0);
  if (ft->vertex_kind) T.vk.assign(ft->vertex_kind, ft->vertex_kind + nV);
  if (ft->edge_kind) T.ek.assign(ft->edge_kind, ft->edge_kind + nE);
  for (int v = 0; v < nV; v++)
    if (T.vk[v] > 1) return set_err(ctx, CGMR_E_INVALID, "%s: vertex %d has kind %d (0 = SE2 pose, 1 = point)", who, v, (int)T.vk[v]);
  std::vector<int32_t> cnt((size_t)std::max(nV, 0) + 1, 0);
  int n_prior = 0;
  for (int k = 0; k < nE; k++) {
    const int kind = T.ek[k], a = ef[k], b = et[k];
    if (a < 0 || a >= nV || b < 0 || b >= nV) return set_err(ctx, CGMR_E_INVALID, "%s: edge %d has a vertex index out of range", who, k);
    if (kind > CGMR_EDGE_PRIOR_SE2_XY) return set_err(ctx, CGMR_E_INVALID, "%s: edge %d has unknown kind %d", who, k, kind);
    if (kind == CGMR_EDGE_SE2_XY || kind == CGMR_EDGE_BEARING_SE2_XY) {
      if (T.vk[a] != 0 || T.vk[b] != 1)
        return set_err(ctx, CGMR_E_INVALID, "%s: edge %d (%s) must go from a pose to a point", who, k, kind == CGMR_EDGE_SE2_XY ? "EDGE_SE2_XY" : "EDGE_BEARING_SE2_XY");
    } else {
      if (T.vk[a] != 0 || T.vk[b] != 0)
        return set_err(ctx, CGMR_E_INVALID, "%s: edge %d (kind %d) touches a point; only EDGE_SE2_XY and EDGE_BEARING_SE2_XY may", who, k, kind);
      if (factor_is_prior(kind)) {
        if (a != b) return set_err(ctx, CGMR_E_INVALID, "%s: edge %d is a prior (kind %d) and must have from == to", who, k, kind);
        cnt[a + 1]++;
        n_prior++;
      }
    }
    if (kind) T.any = true;
  }
  if (!T.any) return 0;
  // CSR of the priors by vertex: vertices ascending, a vertex's edges ascending
  std::vector<int32_t> slot((size_t)nV, -1);
  for (int v = 0; v < nV; v++)
    if (cnt[v + 1]) { slot[v] = (int32_t)T.uv_vertex.size(); T.uv_vertex.push_back(v); T.uv_ptr.push_back(0); }
  T.uv_ptr.push_back(0);
  for (size_t u = 0; u < T.uv_vertex.size(); u++) T.uv_ptr[u + 1] = T.uv_ptr[u] + cnt[T.uv_vertex[u] + 1];
  T.uv_edge.assign((size_t)n_prior, 0);
  std::vector<int32_t> cur(T.uv_ptr.begin(), T.uv_ptr.end());
  for (int k = 0; k < nE; k++) if (factor_is_prior(T.ek[k])) T.uv_edge[cur[slot[ef[k]]]++] = k;
  return 0;
}
// ... staged through ty_arena into Ed (nothing when every kind is zero)
static int typed_upload(cgmr_ctx* ctx, const TypedHost* T, GnEdges& Ed) {
  if (!T || !T->any) return 0;
  Layout256 L;
  const size_t nU = T->uv_vertex.size();
  const size_t o_ek = L.add(T->ek.size()), o_uv = L.add(4 * std::max<size_t>(nU, 1)), o_up = L.add(4 * (nU + 1)),
               o_ue = L.add(4 * std::max<size_t>(T->uv_edge.size(), 1));
  int rc = arena_reserve(ctx, ctx->ty_arena, L.off + 256);
  if (rc) return rc;
  char* d = ctx->ty_arena.ptr;
  hipStream_t st = ctx->stream;
  // (pageable host memory: the copies have left the vectors when they return)
  HIP_TRY(ctx, hipMemcpyAsync(d + o_ek, T->ek.data(), T->ek.size(), hipMemcpyHostToDevice, st));
  if (nU > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(d + o_uv, T->uv_vertex.data(), 4 * nU, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d + o_up, T->uv_ptr.data(), 4 * (nU + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d + o_ue, T->uv_edge.data(), 4 * T->uv_edge.size(), hipMemcpyHostToDevice, st));
  }
  Ed.typed = true;
  Ed.ty.edge_kind = (const uint8_t*)(d + o_ek);
  Ed.unary = {(int)nU, (const int32_t*)(d + o_uv), (const int32_t*)(d + o_up), (const int32_t*)(d + o_ue)};
  return 0;
}
// a point's dummy unknown out of a 3x3 block of H^-1: third row (the block's row vertex is a point) / third column (its column vertex is)
static void zero_point_dims(double* blk, bool row_point, bool col_point) {
  if (row_point) blk[6] = blk[7] = blk[8] = 0.0;
  if (col_point) blk[2] = blk[5] = blk[8] = 0.0;
}

// What a marginals entry point does around its own launches, whichever blocks of H^-1 it is after: the robust description, a
// private copy of the poses, the structure and the masks, the head of the staging block (poses | meas | info; the driver
// adds its own fields to L behind it), one pass that keeps the factor with what reads it, the statistics and the ending.
struct MargCall {
  cgmr_ctx* ctx;
  int nV, nE;
  const cgmr_robust* rk;
  GnEdges Ed;
  std::vector<double> work;          // pushState: the caller's poses stay untouched
  Layout256 L;
  size_t o_p, o_m, o_i;
  char* d = nullptr;                 // the staging block on the device and the poses in it, from stage() on
  double* dp = nullptr;
  bool factor = true;                // false: no free vertex, nothing to factor -- run() queues no pass, close() reads no statistics
  int status4[4] = {0, 0, 0, 0};

  MargCall(cgmr_ctx* c, int nv, const double* poses, int ne, const cgmr_robust* r)
      : ctx(c), nV(nv), nE(ne), rk(r), work(poses, poses + 3 * (size_t)nv), o_p(L.add(24 * (size_t)nv)), o_m(L.add(24 * (size_t)ne)),
        o_i(L.add(48 * (size_t)ne)) {}
  // robust kernels: rho1 at the pass's linearisation point
  int open(const char* who, const TypedHost* typed = nullptr) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = robust_setup(ctx, rk, nE, false, Ed, who);
    return rc ? rc : typed_upload(ctx, typed, Ed);
  }
  int structure(const uint8_t* fixed, const int32_t* ef, const int32_t* et) {
    const int rc = prepare_structure(ctx, nV, nE, ef, et, 1);
    return rc ? rc : prepare_pass(ctx, fixed, nE, ef, et, nE);
  }
  // the staging block as L describes it by now; the head goes up
  int stage(const double* meas, const double* info) {
    const int rc = arena_reserve(ctx, ctx->io_arena, L.off + 256);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    d = ctx->io_arena.ptr;
    dp = (double*)(d + o_p);
    HIP_TRY(ctx, hipMemcpyAsync(dp, work.data(), 24 * (size_t)nV, hipMemcpyHostToDevice, st));
    if (nE > 0) {
      HIP_TRY(ctx, hipMemcpyAsync(d + o_m, meas, 24 * (size_t)nE, hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, hipMemcpyAsync(d + o_i, info, 48 * (size_t)nE, hipMemcpyHostToDevice, st));
    }
    Ed.meas_a = (const double*)(d + o_m); Ed.info_a = (const double*)(d + o_i); Ed.nA = nE; Ed.n_active = nE;
    return 0;
  }
  // gn_pass(.., write_l11c) at dp, then queue(): the driver's launches that read the factor and its result copies; the status
  // words come back with them.
  template <typename Queue>
  int run(GnPassOpts pass, Queue&& queue) {
    GnDevice& D = ctx->gn;
    hipStream_t st = ctx->stream;
    pass.write_l11c = true;
    auto once = [&]() -> int {
      if (factor) gn_pass(ctx, dp, Ed, pass);
      const int rc = queue();
      if (rc) return rc;
      if (factor) HIP_TRY(ctx, hipMemcpyAsync(status4, D.status, sizeof status4, hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));
      HIP_TRY(ctx, hipGetLastError());
      return 0;
    };
    int rc = once();
    if (rc || status4[2] == 0) return rc;
    // A bounded wait ran out (status[2]): a hand-off between workgroups of a merged level launch (the forward pass: factor
    // work items -> update tiles) or of the chained backward solve that never arrived -- not a numerical failure.  As gn_run
    // does, the pass is repeated from the same poses with one launch per kernel and level (no in-kernel waits).  The cached
    // structure keeps only the forward merges that are certainly resident from now on; the chained backward solve (mode 2)
    // stays, as in gn_run: its waits are bounded as well, and a later time-out there falls back the same way.
    choose_fwd_merge(D, ctx->side_used ? 2 : 1, false, false);
    LevelwiseScope levelwise(ctx, D);                             // (ends with those merges and the chained solve back)
    rc = levelwise.arm(st);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(dp, work.data(), 24 * (size_t)nV, hipMemcpyHostToDevice, st));
    rc = once();
    if (rc) return rc;
    if (status4[2] != 0)
      return set_err(ctx, CGMR_E_TIMEOUT, "marginals: a bounded device-side wait (forward hand-off or chained backward solve) ran out twice");
    return 0;
  }
  // the statistics (also after a failed Cholesky: e2 / rho1 of that H), then the factorisation's verdict
  int close() {
    const int rc = factor ? robust_stats_out(ctx, rk, nE, Ed) : 0;
    if (rc) return rc;
    if (status4[0] != 0) return set_err(ctx, CGMR_E_CHOLESKY_BASE, "Cholesky failed while computing marginals");
    return 0;
  }
};

// Shared driver of cgmr_marginals / cgmr_covariance_estimate / cgmr_condense (host pointers).
//   mode 0: marginals at `poses` with `fixed`;  mode 1: covariance estimate (gauge);  mode 2: condense (gauge)
int marginal_driver(cgmr_ctx* ctx, int mode, int nV, const double* poses, const uint8_t* fixed_in, int nE,
                    const int32_t* ef, const int32_t* et, const double* meas, const double* info, int gauge, int nK,
                    const int32_t* query, int32_t* to_out, double* est_out, double* info_out, double* cov_out,
                    const cgmr_robust* rk, const cgmr_factor_types* ft = nullptr) {
  if (nV <= 0 || nE < 0 || nK < 0 || !poses || (nE > 0 && (!ef || !et || !meas || !info)) || (nK > 0 && !query))
    return set_err(ctx, CGMR_E_INVALID, "marginals: null or negative argument");
  if (mode != 0 && (gauge < 0 || gauge >= nV)) return set_err(ctx, CGMR_E_INVALID, "gauge index out of range");
  for (int k = 0; k < nK; k++)
    if (query[k] < 0 || query[k] >= nV) return set_err(ctx, CGMR_E_INVALID, "query index out of range");
  // (the linearisation point: the poses given, or the spanning-tree guess of modes 1 and 2)
  TypedHost typed;                                                      // (mode 0 only: cgmr_marginals_typed)
  int rc = typed_check(ctx, "cgmr_marginals_typed", ft, nV, nE, ef, et, typed);
  if (rc) return rc;
  MargCall call(ctx, nV, poses, nE, rk);
  rc = call.open(ft ? "cgmr_marginals_typed" : mode == 0 ? "cgmr_marginals_robust" : mode == 1 ? "cgmr_covariance_estimate_robust" : "cgmr_condense_robust", &typed);
  if (rc) return rc;
  std::vector<uint8_t> fixed(nV, 0);
  if (mode == 0) { if (!fixed_in) return set_err(ctx, CGMR_E_INVALID, "fixed flags missing"); fixed.assign(fixed_in, fixed_in + nV); }
  else {
    fixed[gauge] = 1;                                                   // fixGauge: every other vertex is freed
    initial_guess_host(nV, call.work.data(), fixed.data(), nE, ef, et, meas);
  }
  // query list (condense: everything but the gauge)
  std::vector<int32_t> q;
  for (int k = 0; k < nK; k++) if (mode != 2 || query[k] != gauge) q.push_back(query[k]);
  const int nq = (int)q.size();
  if (cov_out && mode != 2) memset(cov_out, 0, sizeof(double) * 9 * (size_t)nK);
  rc = call.structure(fixed.data(), ef, et);
  if (rc) return rc;
  Symbolic& S = ctx->sym;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  if (D.nf == 0 || nq == 0) { HIP_TRY(ctx, hipStreamSynchronize(st)); return mode == 2 ? 0 : CGMR_OK; }
  // staging: poses | meas | info | the marginals' and labels' work space
  const MargLayout M(nq, D.nf, S.rows.size(), D.nfronts, call.L.off);
  call.L.off = M.end;
  rc = call.stage(meas, info);
  if (rc) return rc;
  char* d = call.d;
  std::vector<int32_t> qcol(nq);
  for (int k = 0; k < nq; k++) qcol[k] = ctx->vmask[q[k]] ? -1 : S.vperm[q[k]];     // fixed / inactive: zeros
  HIP_TRY(ctx, hipMemcpyAsync(d + M.o_qc, qcol.data(), 4 * (size_t)nq, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + M.o_qv, q.data(), 4 * (size_t)nq, hipMemcpyHostToDevice, st));
  // the Hessian of this iteration (linearised at the initial guess) is what computeMarginals sees [g2o-recalled];
  // for the condensed graph the iteration is completed first: the factor stays valid, the poses move on
  std::vector<double> cov(9 * (size_t)nq);
  GnPassOpts pass;
  pass.solve = pass.update_poses = mode == 2;
  rc = call.run(pass, [&]() -> int {
    launch_marginals(st, D, nq, (const int32_t*)(d + M.o_qc), M.m, (double*)(d + M.o_Y), (double*)(d + M.o_U), (double*)(d + M.o_part),
                     (double*)(d + M.o_G), (double*)(d + M.o_cov), M.chunk, M.nchunk, (uint8_t*)(d + M.o_live));
    if (mode == 2)
      launch_label(st, nq, (const int32_t*)(d + M.o_qv), gauge, call.dp, (const double*)(d + M.o_cov), (double*)(d + M.o_est),
                   (double*)(d + M.o_info), (int*)(d + M.o_fl));
    HIP_TRY(ctx, hipMemcpyAsync(cov.data(), d + M.o_cov, 72 * (size_t)nq, hipMemcpyDeviceToHost, st));
    if (mode == 2) {
      HIP_TRY(ctx, hipMemcpyAsync(est_out, d + M.o_est, 24 * (size_t)nq, hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipMemcpyAsync(info_out, d + M.o_info, 48 * (size_t)nq, hipMemcpyDeviceToHost, st));
    }
    return 0;
  });
  if (rc) return rc;
  rc = call.close();
  if (rc) return rc;
  if (mode == 2) {
    for (int k = 0; k < nq; k++) to_out[k] = q[k];
    if (cov_out) memcpy(cov_out, cov.data(), 72 * (size_t)nq);
    return nq;
  }
  // scatter back in query order; fixed / inactive queries keep zeros
  for (int k = 0; k < nq; k++)
    if (qcol[k] >= 0) {
      memcpy(cov_out + 9 * (size_t)k, cov.data() + 9 * (size_t)k, 72);
      if (typed.any && typed.vk[q[k]]) zero_point_dims(cov_out + 9 * (size_t)k, true, true);
    }
  return CGMR_OK;
}

// cgmr_marginals_all: Sigma of every front by selected inversion of the factor (selinv_kernels.hip), then the diagonal block
// of every vertex and the block of every edge.  The same pass as marginal_driver's mode 0 (gn_pass at `poses` with `fixed`).
int marginals_all_driver(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                         const int32_t* et, const double* meas, const double* info, double* cov_out, double* cross_out,
                         const cgmr_robust* rk, const cgmr_factor_types* ft = nullptr) {
  if (nV <= 0 || nE < 0 || !poses || !cov_out || (nE > 0 && (!ef || !et || !meas || !info)))
    return set_err(ctx, CGMR_E_INVALID, "marginals: null or negative argument");
  if (!fixed) return set_err(ctx, CGMR_E_INVALID, "fixed flags missing");
  TypedHost typed;
  int rc = typed_check(ctx, "cgmr_marginals_all_typed", ft, nV, nE, ef, et, typed);
  if (rc) return rc;
  MargCall call(ctx, nV, poses, nE, rk);
  rc = call.open(ft ? "cgmr_marginals_all_typed" : "cgmr_marginals_all_robust", &typed);
  if (rc) return rc;
  auto zero_outputs = [&]() {
    memset(cov_out, 0, 72 * (size_t)nV);
    if (cross_out) memset(cross_out, 0, 72 * (size_t)nE);
  };
  zero_outputs();
  rc = call.structure(fixed, ef, et);
  if (rc) return rc;
  Symbolic& S = ctx->sym;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  if (D.nf == 0) { HIP_TRY(ctx, hipStreamSynchronize(st)); return CGMR_OK; }
  // every front's block of Sigma (own columns, then the border), and the row tiles of k_selinv_border level by level
  const int nfr = (int)S.fronts.size();
  std::vector<int64_t> soff(nfr + 1, 0);
  for (int f = 0; f < nfr; f++) {
    const int64_t n = 3 * (int64_t)(S.fronts[f].nc + S.fronts[f].ns);
    soff[f + 1] = soff[f] + n * n;
  }
  SelinvPlan P;
  std::vector<int32_t> tiles;
  P.h_tile_ptr.assign(D.nlevels_full + 1, 0);
  for (int l = 0; l < D.nlevels_full; l++) {
    for (int q = D.h_flevel_ptr[l]; q < D.h_flevel_ptr[l + 1]; q++) {
      const int f = S.level_fronts[q];
      if (S.fronts[f].parent < 0) continue;                             // (a root has no border)
      for (int t0 = 0; t0 < 3 * S.fronts[f].ns; t0 += kSelinvTileRows) { tiles.push_back(f); tiles.push_back(t0); }
    }
    P.h_tile_ptr[l + 1] = (int)tiles.size() / 2;
  }
  std::vector<int32_t> vcol(nV);
  for (int v = 0; v < nV; v++) vcol[v] = ctx->vmask[v] ? -1 : S.vperm[v];     // fixed / inactive: zeros
  // staging: poses | meas | info | vcol | col_front | soff | tiles | cov | cross;  Sigma: an arena of its own
  Layout256& L = call.L;
  const size_t o_vc = L.add(4 * (size_t)nV), o_cf = L.add(4 * (size_t)D.nf), o_so = L.add(8 * soff.size()), o_t = L.add(4 * tiles.size()),
               o_cov = L.add(72 * (size_t)nV), o_cr = L.add(72 * (size_t)nE);
  rc = arena_reserve(ctx, ctx->si_arena, 8 * (size_t)soff[nfr]);
  if (rc) return rc;
  rc = call.stage(meas, info);
  if (rc) return rc;
  char* d = call.d;
  HIP_TRY(ctx, hipMemcpyAsync(d + o_vc, vcol.data(), 4 * (size_t)nV, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_cf, S.col_front.data(), 4 * (size_t)D.nf, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_so, soff.data(), 8 * soff.size(), hipMemcpyHostToDevice, st));
  if (!tiles.empty()) HIP_TRY(ctx, hipMemcpyAsync(d + o_t, tiles.data(), 4 * tiles.size(), hipMemcpyHostToDevice, st));
  P.Sig = (double*)ctx->si_arena.ptr;
  P.soff = (const int64_t*)(d + o_so);
  P.tiles = (const int32_t*)(d + o_t);
  GnPassOpts pass;
  pass.solve = false;
  rc = call.run(pass, [&]() -> int {
    launch_invert_fronts(st, D, /*top_too=*/true);                     // Z = L11^-1 of every front, the top block's included
    launch_selinv(st, D, P, nV, nE, (const int32_t*)(d + o_vc), (const int32_t*)(d + o_cf), (double*)(d + o_cov),
                  cross_out ? (double*)(d + o_cr) : nullptr);
    HIP_TRY(ctx, hipMemcpyAsync(cov_out, d + o_cov, 72 * (size_t)nV, hipMemcpyDeviceToHost, st));
    if (cross_out && nE > 0) HIP_TRY(ctx, hipMemcpyAsync(cross_out, d + o_cr, 72 * (size_t)nE, hipMemcpyDeviceToHost, st));
    return 0;
  });
  if (rc) return rc;
  rc = call.close();
  if (rc == CGMR_E_CHOLESKY_BASE) zero_outputs();
  if (rc == CGMR_OK && typed.any) {
    for (int v = 0; v < nV; v++) if (typed.vk[v]) zero_point_dims(cov_out + 9 * (size_t)v, true, true);
    if (cross_out) for (int k = 0; k < nE; k++) zero_point_dims(cross_out + 9 * (size_t)k, typed.vk[ef[k]] != 0, typed.vk[et[k]] != 0);
  }
  return rc;
}

// Shared driver of cgmr_marginals_joint / cgmr_marginals_pairs / cgmr_relative_covariance, their typed forms and
// cgmr_observation_covariance (`who`): the pass of marginal_driver's mode 0
// (gn_pass at `poses` with `fixed`), the solve half of launch_marginals for the unique vertices asked for, then the tiles of
// Y^T Y that hold a requested block (joint_marginals_kernels.hip).
//   mode 0: joint -- va = the nK queries, out_a = cov [(3 nK)^2]
//   mode 1: pairs -- (va, vb) the nP pairs, out_a / out_b / out_c = aa / ab / bb (nullable)
//   mode 2: relative covariance -- the pairs' blocks stay on the device; out_a / out_b / out_c = rel_xyt / rel_cov / d2 (nullable);
//           obs: cgmr_observation_covariance, pair p predicted as a factor of kind obs_kind[p] (null: all 0).  The pairs of
//           kind 0 are k_relative_cov's (it runs over the whole list when there is one), the others k_observation_cov's behind it.
// ft: the factor types (typed_check before the device is touched; a point's dummy third row / column comes back zero).
int joint_driver(cgmr_ctx* ctx, const char* who, int mode, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                 const int32_t* et, const double* meas, const double* info, int nQ, const int32_t* va, const int32_t* vb,
                 double* out_a, double* out_b, double* out_c, const double* hyp_meas, const double* hyp_info,
                 const cgmr_robust* rk, const cgmr_factor_types* ft = nullptr, bool obs = false, const uint8_t* obs_kind = nullptr) {
  if (nV <= 0 || nE < 0 || nQ < 0 || !poses || !fixed || (nE > 0 && (!ef || !et || !meas || !info)) ||
      (nQ > 0 && (!va || (mode != 0 && !vb))) || (mode == 0 && nQ > 0 && !out_a) || (mode == 2 && ((out_c && !hyp_meas) || (hyp_info && !hyp_meas))))
    return set_err(ctx, CGMR_E_INVALID, "%s: null or negative argument", who);
  for (int k = 0; k < nQ; k++)
    if (va[k] < 0 || va[k] >= nV || (mode != 0 && (vb[k] < 0 || vb[k] >= nV)))
      return set_err(ctx, CGMR_E_INVALID, "%s: vertex index out of range", who);
  TypedHost typed;
  int rc = typed_check(ctx, who, ft, nV, nE, ef, et, typed);
  if (rc) return rc;
  bool obs_typed = false, obs_pose = !obs;                        // some pair is a landmark observation / a relative pose
  if (obs)
    for (int k = 0; k < nQ; k++) {
      const int kind = obs_kind ? obs_kind[k] : 0;
      const bool a_pt = ft && !typed.vk.empty() && typed.vk[va[k]], b_pt = ft && !typed.vk.empty() && typed.vk[vb[k]];
      if (kind > CGMR_EDGE_BEARING_SE2_XY) return set_err(ctx, CGMR_E_INVALID, "%s: pair %d has observation kind %d (0, 1 or 2)", who, k, kind);
      if (a_pt) return set_err(ctx, CGMR_E_INVALID, "%s: pair %d is observed from vertex %d, a point", who, k, va[k]);
      if (kind == CGMR_EDGE_SE2 && b_pt) return set_err(ctx, CGMR_E_INVALID, "%s: pair %d of kind 0 (EDGE_SE2) ends at vertex %d, a point", who, k, vb[k]);
      if (kind != CGMR_EDGE_SE2 && !b_pt) return set_err(ctx, CGMR_E_INVALID, "%s: pair %d of kind %d ends at vertex %d, a pose", who, k, kind, vb[k]);
      if (kind) obs_typed = true; else obs_pose = true;
    }
  if (nQ == 0) return CGMR_OK;
  // the unique vertices, in order of first appearance: 4 columns of Y each
  std::vector<int32_t> slot_of(nV, -1), uq;
  auto slot = [&](int v) { if (slot_of[v] < 0) { slot_of[v] = (int32_t)uq.size(); uq.push_back(v); } return slot_of[v]; };
  for (int k = 0; k < nQ; k++) { slot(va[k]); if (mode != 0) slot(vb[k]); }
  const int nU = (int)uq.size();
  if (nU > CGMR_JOINT_MAX_QUERIES)
    return set_err(ctx, CGMR_E_INVALID, "%s: %d unique query vertices, at most CGMR_JOINT_MAX_QUERIES = %d", who, nU, CGMR_JOINT_MAX_QUERIES);
  MargCall call(ctx, nV, poses, nE, rk);
  rc = call.open(who, &typed);
  if (rc) return rc;
  rc = call.structure(fixed, ef, et);
  if (rc) return rc;
  Symbolic& S = ctx->sym;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  const size_t nq = (size_t)nQ;
  const size_t b_a = mode == 0 ? 72 * nq * nq : mode == 1 ? 72 * nq : 24 * nq, b_b = 72 * nq, b_c = mode == 1 ? 72 * nq : 8 * nq;
  auto zero_outputs = [&]() {
    if (out_a) memset(out_a, 0, b_a);
    if (mode != 0 && out_b) memset(out_b, 0, b_b);
    if (mode != 0 && out_c) memset(out_c, 0, b_c);
  };
  if (D.nf == 0 && mode != 2) { HIP_TRY(ctx, hipStreamSynchronize(st)); zero_outputs(); return CGMR_OK; }   // no free vertex: zeros
  call.factor = D.nf > 0;
  // the tiles: every lower one (joint), or those of the pairs' blocks, sorted, each once
  const MargLayout M(nU, D.nf, S.rows.size(), D.nfronts, 0);
  const int T = M.m / 16;
  std::vector<int32_t> qcol(nU), tl, pr;
  for (int k = 0; k < nU; k++) qcol[k] = ctx->vmask[uq[k]] ? -1 : S.vperm[uq[k]];      // fixed / inactive: zero columns
  JointGram JG;
  if (mode == 0) {
    JG.ntile = (long long)T * (T + 1) / 2;
    pr.resize(nQ);
    for (int k = 0; k < nQ; k++) pr[k] = qcol[slot_of[va[k]]] < 0 ? -1 : slot_of[va[k]];
  } else {
    std::vector<int64_t> keys;
    keys.reserve(3 * nq);
    auto key = [&](int sa, int sb) { const int I = std::max(sa, sb) / 4, J = std::min(sa, sb) / 4; return (int64_t)I * T + J; };
    for (int k = 0; k < nQ; k++) {
      const int sa = slot_of[va[k]], sb = slot_of[vb[k]];
      keys.push_back(key(sa, sa)); keys.push_back(key(sa, sb)); keys.push_back(key(sb, sb));
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    JG.ntile = (long long)keys.size();
    tl.resize(2 * keys.size());
    for (size_t t = 0; t < keys.size(); t++) { tl[2 * t] = (int32_t)(keys[t] / T); tl[2 * t + 1] = (int32_t)(keys[t] % T); }
    auto pos = [&](int sa, int sb) { return (int32_t)(std::lower_bound(keys.begin(), keys.end(), key(sa, sb)) - keys.begin()); };
    pr.resize(5 * nq);
    for (int k = 0; k < nQ; k++) {
      const int sa = slot_of[va[k]], sb = slot_of[vb[k]];
      int32_t* P = &pr[5 * (size_t)k];
      P[0] = qcol[sa] < 0 ? -1 : sa; P[1] = qcol[sb] < 0 ? -1 : sb;
      P[2] = pos(sa, sa); P[3] = pos(sa, sb); P[4] = pos(sb, sb);
    }
  }
  const long long nwg = mode == 0 ? (long long)((T + 3) / 4) * ((T + 3) / 4 + 1) / 2 : JG.ntile;
  joint_gram_split(M.n, nwg, &JG.rows, &JG.nsplit);
  // staging: poses | meas | info | query columns, Y, border vectors, live flags (MargLayout) | tile list | pairs / slots |
  // partial tiles | tiles | outputs | the pair vertices and the hypotheses
  Layout256& L = call.L;
  const MargLayout ML(nU, D.nf, S.rows.size(), D.nfronts, L.off);
  L.off = ML.end;
  const size_t o_tl = L.add(4 * tl.size()), o_pr = L.add(4 * pr.size()),
               o_part = L.add(JG.nsplit > 1 ? 2048 * (size_t)JG.nsplit * (size_t)JG.ntile : 0), o_G = L.add(2048 * (size_t)JG.ntile),
               o_a = L.add(mode == 0 ? 72 * nq * nq : 72 * nq), o_b = L.add(mode == 0 ? 0 : 72 * nq), o_c = L.add(mode == 0 ? 0 : 72 * nq),
               o_va = L.add(mode == 2 ? 4 * nq : 0), o_vb = L.add(mode == 2 ? 4 * nq : 0), o_hm = L.add(mode == 2 && hyp_meas ? 24 * nq : 0),
               o_hi = L.add(mode == 2 && hyp_info ? 48 * nq : 0), o_rz = L.add(mode == 2 ? 24 * nq : 0), o_rc = L.add(mode == 2 ? 72 * nq : 0),
               o_d2 = L.add(mode == 2 ? 8 * nq : 0), o_ok = L.add(obs_typed ? nq : 0);
  rc = call.stage(meas, info);
  if (rc) return rc;
  char* d = call.d;
  HIP_TRY(ctx, hipMemcpyAsync(d + ML.o_qc, qcol.data(), 4 * (size_t)nU, hipMemcpyHostToDevice, st));
  if (!tl.empty()) HIP_TRY(ctx, hipMemcpyAsync(d + o_tl, tl.data(), 4 * tl.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_pr, pr.data(), 4 * pr.size(), hipMemcpyHostToDevice, st));
  if (mode == 2) {
    HIP_TRY(ctx, hipMemcpyAsync(d + o_va, va, 4 * nq, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d + o_vb, vb, 4 * nq, hipMemcpyHostToDevice, st));
    if (hyp_meas) HIP_TRY(ctx, hipMemcpyAsync(d + o_hm, hyp_meas, 24 * nq, hipMemcpyHostToDevice, st));
    if (hyp_info) HIP_TRY(ctx, hipMemcpyAsync(d + o_hi, hyp_info, 48 * nq, hipMemcpyHostToDevice, st));
    if (obs_typed) HIP_TRY(ctx, hipMemcpyAsync(d + o_ok, obs_kind, nq, hipMemcpyHostToDevice, st));
  }
  JG.tiles = mode == 0 ? nullptr : (const int32_t*)(d + o_tl);
  JG.part = (double*)(d + o_part);
  JG.G = (double*)(d + o_G);
  GnPassOpts pass;
  pass.solve = pass.update_poses = false;
  const bool want_d2 = mode == 2 && out_c;
  rc = call.run(pass, [&]() -> int {
    if (call.factor) {
      launch_marginals_solve(st, D, nU, (const int32_t*)(d + ML.o_qc), ML.m, (double*)(d + ML.o_Y), (double*)(d + ML.o_U),
                             (uint8_t*)(d + ML.o_live));
      launch_joint_gram(st, ML.n, ML.m, (const double*)(d + ML.o_Y), JG);
      if (mode == 0) launch_joint_extract(st, nQ, (const int32_t*)(d + o_pr), JG.G, (double*)(d + o_a));
      else launch_pairs_extract(st, nQ, (const int32_t*)(d + o_pr), JG.G, (double*)(d + o_a), (double*)(d + o_b), (double*)(d + o_c));
    } else {                                                           // (mode 2 without a free vertex: zero blocks)
      HIP_TRY(ctx, hipMemsetAsync(d + o_a, 0, 72 * nq, st));
      HIP_TRY(ctx, hipMemsetAsync(d + o_b, 0, 72 * nq, st));
      HIP_TRY(ctx, hipMemsetAsync(d + o_c, 0, 72 * nq, st));
    }
    if (mode == 0) HIP_TRY(ctx, hipMemcpyAsync(out_a, d + o_a, b_a, hipMemcpyDeviceToHost, st));
    if (mode == 1) {
      if (out_a) HIP_TRY(ctx, hipMemcpyAsync(out_a, d + o_a, b_a, hipMemcpyDeviceToHost, st));
      if (out_b) HIP_TRY(ctx, hipMemcpyAsync(out_b, d + o_b, b_b, hipMemcpyDeviceToHost, st));
      if (out_c) HIP_TRY(ctx, hipMemcpyAsync(out_c, d + o_c, b_c, hipMemcpyDeviceToHost, st));
    }
    if (mode == 2 && obs_pose)
      launch_relative_cov(st, nQ, (const int32_t*)(d + o_va), (const int32_t*)(d + o_vb), call.dp, (const double*)(d + o_a),
                          (const double*)(d + o_b), (const double*)(d + o_c), hyp_meas ? (const double*)(d + o_hm) : nullptr,
                          hyp_info ? (const double*)(d + o_hi) : nullptr, (double*)(d + o_rz), (double*)(d + o_rc),
                          want_d2 ? (double*)(d + o_d2) : nullptr);
    if (mode == 2 && obs_typed)
      launch_observation_cov(st, nQ, (const int32_t*)(d + o_va), (const int32_t*)(d + o_vb), (const uint8_t*)(d + o_ok), call.dp,
                             (const double*)(d + o_a), (const double*)(d + o_b), (const double*)(d + o_c),
                             hyp_meas ? (const double*)(d + o_hm) : nullptr, hyp_info ? (const double*)(d + o_hi) : nullptr,
                             (double*)(d + o_rz), (double*)(d + o_rc), want_d2 ? (double*)(d + o_d2) : nullptr);
    if (mode == 2) {
      if (out_a) HIP_TRY(ctx, hipMemcpyAsync(out_a, d + o_rz, b_a, hipMemcpyDeviceToHost, st));
      if (out_b) HIP_TRY(ctx, hipMemcpyAsync(out_b, d + o_rc, b_b, hipMemcpyDeviceToHost, st));
      if (want_d2) HIP_TRY(ctx, hipMemcpyAsync(out_c, d + o_d2, b_c, hipMemcpyDeviceToHost, st));
    }
    return 0;
  });
  if (rc) return rc;
  rc = call.close();
  if (rc == CGMR_E_CHOLESKY_BASE) zero_outputs();
  if (rc == CGMR_OK && typed.any && mode == 0) {                  // the points' dummy unknowns: rows and columns 3 k + 2
    const size_t N = 3 * nq;
    for (int k = 0; k < nQ; k++)
      if (typed.vk[va[k]])
        for (size_t q = 0; q < N; q++) out_a[(3 * (size_t)k + 2) * N + q] = out_a[q * N + 3 * (size_t)k + 2] = 0.0;
  }
  if (rc == CGMR_OK && typed.any && mode == 1)
    for (int k = 0; k < nQ; k++) {
      const bool pa = typed.vk[va[k]] != 0, pb = typed.vk[vb[k]] != 0;
      if (out_a) zero_point_dims(out_a + 9 * (size_t)k, pa, pa);
      if (out_b) zero_point_dims(out_b + 9 * (size_t)k, pa, pb);
      if (out_c) zero_point_dims(out_c + 9 * (size_t)k, pb, pb);
    }
  return rc;
}

// What the clique kernels of pcm_kernels.hip work in, behind whatever the caller has put into L: the seeds' member bits and
// sizes and the result (size, seed, members).
struct CliqueLayout {
  size_t o_sb, o_ss, o_out;
  CliqueLayout(Layout256& L, int n) : o_sb(L.add(8 * (size_t)n * ((n + 63) / 64))), o_ss(L.add(4 * (size_t)n)), o_out(L.add(4 * ((size_t)n + 2))) {}
};
// ... and where its result goes on the host once the stream has been waited for (res: n + 2 ints)
static void clique_result_out(const std::vector<int32_t>& res, int n, int32_t* clique_out, int32_t* size_out, int32_t* seed_out) {
  *size_out = res[0];
  *seed_out = res[1];
  memcpy(clique_out, res.data() + 2, 4 * (size_t)n);
}

// cgmr_closure_consistency: the pass and the solve half of joint_driver's mode 0 over the unique endpoints of the candidates,
// every lower Gram tile (the macro-tile path), then the kernels of pcm_kernels.hip on the tiles where they lie: d2 of every
// pair, its rows as bit words, the greedy clique of every seed and the best of them.  In profiling mode the launch classes
// 9 (solve + Gram), 10 (k_closure_consistency) and 11 (bits and clique) of cgmr_gn_kernel_times_ex are timed and collected.
int pcm_driver(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et,
               const double* meas, const double* info, int nC, const int32_t* ca, const int32_t* cb, const double* cmeas,
               const double* cinfo, double gamma, double* d2_out, uint64_t* adj_out, int32_t* clique_out, int32_t* size_out,
               int32_t* seed_out, const cgmr_robust* rk) {
  const char* who = "cgmr_closure_consistency";
  if (nV <= 0 || nE < 0 || nC < 0 || !poses || !fixed || (nE > 0 && (!ef || !et || !meas || !info)) || (nC > 0 && (!ca || !cb || !cmeas || !cinfo)))
    return set_err(ctx, CGMR_E_INVALID, "%s: null or negative argument", who);
  const bool want_clique = clique_out || size_out || seed_out;
  if (want_clique && !(clique_out && size_out && seed_out))
    return set_err(ctx, CGMR_E_INVALID, "%s: clique_out, clique_size_out and seed_out are given together or not at all", who);
  if (nC > CGMR_PCM_MAX_CLOSURES)
    return set_err(ctx, CGMR_E_INVALID, "%s: %d closures, at most CGMR_PCM_MAX_CLOSURES = %d", who, nC, CGMR_PCM_MAX_CLOSURES);
  for (int k = 0; k < nC; k++)
    if (ca[k] < 0 || ca[k] >= nV || cb[k] < 0 || cb[k] >= nV)
      return set_err(ctx, CGMR_E_INVALID, "%s: closure %d (%d -> %d) has an endpoint outside [0, %d)", who, k, ca[k], cb[k], nV);
  if (!(std::isfinite(gamma) && gamma > 0)) return set_err(ctx, CGMR_E_INVALID, "%s: gamma must be finite and > 0", who);
  if (nC == 0) { if (size_out) *size_out = 0; return CGMR_OK; }
  // the unique endpoints, in order of first appearance: 4 columns of Y each (at most 2 nC <= CGMR_JOINT_MAX_QUERIES)
  std::vector<int32_t> slot_of(nV, -1), uq;
  auto slot = [&](int v) { if (slot_of[v] < 0) { slot_of[v] = (int32_t)uq.size(); uq.push_back(v); } return slot_of[v]; };
  for (int k = 0; k < nC; k++) { slot(ca[k]); slot(cb[k]); }
  const int nU = (int)uq.size();
  MargCall call(ctx, nV, poses, nE, rk);
  int rc = call.open(who);
  if (rc) return rc;
  rc = call.structure(fixed, ef, et);
  if (rc) return rc;
  Symbolic& S = ctx->sym;
  GnDevice& D = ctx->gn;
  hipStream_t st = ctx->stream;
  call.factor = D.nf > 0;                                          // no free vertex: Sigma = 0, the measurement terms alone
  const MargLayout M(nU, D.nf, S.rows.size(), D.nfronts, 0);
  const int T = M.m / 16, W = (nC + 63) / 64;
  const size_t n = (size_t)nC;
  std::vector<int32_t> qcol(nU), sl(2 * n);
  for (int k = 0; k < nU; k++) qcol[k] = ctx->vmask[uq[k]] ? -1 : S.vperm[uq[k]];      // fixed / inactive: zero columns
  for (int k = 0; k < nC; k++) {
    const int sa = slot_of[ca[k]], sb = slot_of[cb[k]];
    sl[2 * k] = qcol[sa] < 0 ? -1 : sa; sl[2 * k + 1] = qcol[sb] < 0 ? -1 : sb;
  }
  JointGram JG;
  JG.ntile = (long long)T * (T + 1) / 2;
  joint_gram_split(M.n, (long long)((T + 3) / 4) * ((T + 3) / 4 + 1) / 2, &JG.rows, &JG.nsplit);
  // staging: poses | meas | info | query columns, Y, border vectors, live flags (MargLayout) | partial tiles | tiles | the
  // candidates | d2 | bit words | the clique's work space
  Layout256& L = call.L;
  const MargLayout ML(nU, D.nf, S.rows.size(), D.nfronts, L.off);
  L.off = ML.end;
  const size_t o_part = L.add(JG.nsplit > 1 ? 2048 * (size_t)JG.nsplit * (size_t)JG.ntile : 0), o_G = L.add(2048 * (size_t)JG.ntile),
               o_sl = L.add(8 * n), o_ca = L.add(4 * n), o_cb = L.add(4 * n), o_cm = L.add(24 * n), o_ci = L.add(48 * n),
               o_d2 = L.add(8 * n * n), o_adj = L.add(8 * n * W);
  const CliqueLayout CL(L, nC);
  rc = call.stage(meas, info);
  if (rc) return rc;
  char* d = call.d;
  HIP_TRY(ctx, hipMemcpyAsync(d + ML.o_qc, qcol.data(), 4 * (size_t)nU, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_sl, sl.data(), 8 * n, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_ca, ca, 4 * n, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_cb, cb, 4 * n, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_cm, cmeas, 24 * n, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_ci, cinfo, 48 * n, hipMemcpyHostToDevice, st));
  JG.part = (double*)(d + o_part);
  JG.G = (double*)(d + o_G);
  PcmClosures C;
  C.n = nC;
  C.a = (const int32_t*)(d + o_ca); C.b = (const int32_t*)(d + o_cb); C.slot = (const int32_t*)(d + o_sl);
  C.meas = (const double*)(d + o_cm); C.info = (const double*)(d + o_ci);
  std::vector<int32_t> res(n + 2, 0);
  GnPassOpts pass;
  pass.solve = pass.update_poses = false;
  rc = call.run(pass, [&]() -> int {
    KTimer KT{ctx, st};
    if (call.factor)
      KT.run(9, 2, [&] {
        launch_marginals_solve(st, D, nU, (const int32_t*)(d + ML.o_qc), ML.m, (double*)(d + ML.o_Y), (double*)(d + ML.o_U),
                               (uint8_t*)(d + ML.o_live));
        launch_joint_gram(st, ML.n, ML.m, (const double*)(d + ML.o_Y), JG);
      });
    KT.run(10, 1, [&] { launch_closure_consistency(st, C, call.dp, JG.G, (double*)(d + o_d2)); });
    if (adj_out || want_clique)
      KT.run(11, want_clique ? 3 : 1, [&] {
        launch_consistency_bits(st, nC, (const double*)(d + o_d2), gamma, (unsigned long long*)(d + o_adj));
        if (want_clique)
          launch_clique_greedy(st, nC, (const unsigned long long*)(d + o_adj), (unsigned long long*)(d + CL.o_sb), (int32_t*)(d + CL.o_ss),
                               (int32_t*)(d + CL.o_out));
      });
    if (d2_out) HIP_TRY(ctx, hipMemcpyAsync(d2_out, d + o_d2, 8 * n * n, hipMemcpyDeviceToHost, st));
    if (adj_out) HIP_TRY(ctx, hipMemcpyAsync(adj_out, d + o_adj, 8 * n * W, hipMemcpyDeviceToHost, st));
    if (want_clique) HIP_TRY(ctx, hipMemcpyAsync(res.data(), d + CL.o_out, 4 * (n + 2), hipMemcpyDeviceToHost, st));
    return 0;
  });
  if (ctx->profiling) profile_collect(ctx);
  if (rc) return rc;
  rc = call.close();
  if (rc == CGMR_E_CHOLESKY_BASE) {
    if (d2_out) memset(d2_out, 0, 8 * n * n);
    if (adj_out) memset(adj_out, 0, 8 * n * W);
    std::fill(res.begin(), res.end(), 0);
  }
  if (want_clique && (rc == CGMR_OK || rc == CGMR_E_CHOLESKY_BASE)) clique_result_out(res, nC, clique_out, size_out, seed_out);
  return rc;
}

// cgmr_max_clique_greedy: the clique kernels alone on a caller's adjacency words, checked on the host first
int clique_driver(cgmr_ctx* ctx, int n, const uint64_t* adj, int32_t* clique_out, int32_t* size_out, int32_t* seed_out) {
  const char* who = "cgmr_max_clique_greedy";
  if (n < 0 || !size_out || (n > 0 && (!adj || !clique_out || !seed_out))) return set_err(ctx, CGMR_E_INVALID, "%s: null or negative argument", who);
  if (n > CGMR_PCM_MAX_CLOSURES) return set_err(ctx, CGMR_E_INVALID, "%s: %d vertices, at most CGMR_PCM_MAX_CLOSURES = %d", who, n, CGMR_PCM_MAX_CLOSURES);
  if (n == 0) { *size_out = 0; return CGMR_OK; }
  const int W = (n + 63) / 64;
  auto bit = [&](int k, int l) { return (int)((adj[(size_t)k * W + (l >> 6)] >> (l & 63)) & 1u); };
  for (int k = 0; k < n; k++) {
    if (bit(k, k)) return set_err(ctx, CGMR_E_INVALID, "%s: word %d: vertex %d is adjacent to itself", who, k * W + (k >> 6), k);
    if ((n & 63) && (adj[(size_t)k * W + W - 1] >> (n & 63)))
      return set_err(ctx, CGMR_E_INVALID, "%s: word %d: a padding bit (column >= %d) of row %d is set", who, k * W + W - 1, n, k);
    for (int l = 0; l < k; l++)
      if (bit(k, l) != bit(l, k))
        return set_err(ctx, CGMR_E_INVALID, "%s: word %d: bit (%d, %d) differs from bit (%d, %d)", who, k * W + (l >> 6), k, l, l, k);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Layout256 L;
  const size_t o_adj = L.add(8 * (size_t)n * W);
  const CliqueLayout CL(L, n);
  int rc = arena_reserve(ctx, ctx->io_arena, L.off + 256);
  if (rc) return rc;
  char* d = ctx->io_arena.ptr;
  hipStream_t st = ctx->stream;
  std::vector<int32_t> res((size_t)n + 2, 0);
  HIP_TRY(ctx, hipMemcpyAsync(d + o_adj, adj, 8 * (size_t)n * W, hipMemcpyHostToDevice, st));
  KTimer KT{ctx, st};
  KT.run(11, 2, [&] {
    launch_clique_greedy(st, n, (const unsigned long long*)(d + o_adj), (unsigned long long*)(d + CL.o_sb), (int32_t*)(d + CL.o_ss),
                         (int32_t*)(d + CL.o_out));
  });
  HIP_TRY(ctx, hipMemcpyAsync(res.data(), d + CL.o_out, 4 * ((size_t)n + 2), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipGetLastError());
  if (ctx->profiling) profile_collect(ctx);
  clique_result_out(res, n, clique_out, size_out, seed_out);
  return CGMR_OK;
}

// The mixture of a mixture entry point (include/cgmr.h: cgmr_mixture), checked on the host before the device is touched.  `any`:
// some edge has more than one component (none: the call is the typed / plain one on meas / info, bit for bit).  off: per
// component c = max_j a_j - a, a = 2 ln w + ln det Omega over the factor's own dimension, in double on the host; 0 on an edge
// of one component, whose weight and Omega are not looked at.
struct MixHost {
  bool any = false;
  const cgmr_mixture* mix = nullptr;
  size_t nC = 0;
  std::vector<double> off;
};
static int mix_check(cgmr_ctx* ctx, const char* who, const cgmr_mixture* mix, int nE, const TypedHost& typed, MixHost& M) {
  if (!mix || !mix->comp_ptr) return 0;
  const int32_t* cp = mix->comp_ptr;
  if (cp[0] != 0) return set_err(ctx, CGMR_E_INVALID, "%s: comp_ptr[0] must be 0 (edge 0)", who);
  for (int k = 0; k < nE; k++) {
    if (cp[k + 1] <= cp[k])
      return set_err(ctx, CGMR_E_INVALID, "%s: edge %d has no component (comp_ptr must increase from 0)", who, k);
    if (cp[k + 1] - cp[k] > 1) M.any = true;
  }
  if (!M.any) return 0;
  if (!mix->comp_meas || !mix->comp_info || !mix->comp_weight)
    return set_err(ctx, CGMR_E_INVALID, "%s: a mixture needs comp_meas, comp_info and comp_weight", who);
  M.mix = mix;
  M.nC = (size_t)cp[nE];
  M.off.assign(M.nC, 0.0);
  for (int k = 0; k < nE; k++) {
    const int p0 = cp[k], p1 = cp[k + 1];
    if (p1 - p0 < 2) continue;
    const int dim = factor_dim(typed.any ? typed.ek[k] : CGMR_EDGE_SE2);
    double amax = 0;
    for (int p = p0; p < p1; p++) {
      const double w = mix->comp_weight[p];
      const double* u = mix->comp_info + 6 * (size_t)p;
      const double det = dim == 1 ? u[0]
                         : dim == 2
                             ? u[0] * u[3] - u[1] * u[1]
                             : u[0] * (u[3] * u[5] - u[4] * u[4]) - u[1] * (u[1] * u[5] - u[4] * u[2]) + u[2] * (u[1] * u[4] - u[3] * u[2]);
      if (!(std::isfinite(w) && w > 0))
        return set_err(ctx, CGMR_E_INVALID, "%s: edge %d, component %d: the weight must be finite and > 0", who, k, p - p0);
      if (!(std::isfinite(det) && det > 0))
        return set_err(ctx, CGMR_E_INVALID, "%s: edge %d, component %d: det Omega (the factor's own dimension) must be finite and > 0", who, k, p - p0);
      const double a = 2 * std::log(w) + std::log(det);
      M.off[p] = a;
      if (p == p0 || a > amax) amax = a;
    }
    for (int p = p0; p < p1; p++) M.off[p] = amax - M.off[p];
  }
  return 0;
}
// ... staged through mix_arena into Ed (nothing without a multi-component edge); the selection lands behind the lists
static int mix_upload(cgmr_ctx* ctx, const MixHost* M, int nE, GnEdges& Ed) {
  if (!M || !M->any) return 0;
  Layout256 L;
  const size_t nC = M->nC, n = (size_t)nE;
  const size_t o_ptr = L.add(4 * (n + 1)), o_meas = L.add(24 * nC), o_info = L.add(48 * nC), o_off = L.add(8 * nC), o_sel = L.add(4 * n);
  int rc = arena_reserve(ctx, ctx->mix_arena, L.off + 256);
  if (rc) return rc;
  char* d = ctx->mix_arena.ptr;
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipMemcpyAsync(d + o_ptr, M->mix->comp_ptr, 4 * (n + 1), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_meas, M->mix->comp_meas, 24 * nC, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_info, M->mix->comp_info, 48 * nC, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d + o_off, M->off.data(), 8 * nC, hipMemcpyHostToDevice, st));
  Ed.mix = true;
  Ed.mx.cptr = (const int32_t*)(d + o_ptr);
  Ed.mx.cmeas = (const double*)(d + o_meas); Ed.mx.cinfo = (const double*)(d + o_info); Ed.mx.coff = (const double*)(d + o_off);
  Ed.mx.sel_out = M->mix->selected_out ? (int32_t*)(d + o_sel) : nullptr;
  return 0;
}
// every edge's first component: what a call routed to the typed / plain path, or one that fails, leaves in selected_out
static void mix_selection_zero(const cgmr_mixture* mix, int nE) {
  if (mix && mix->selected_out) for (int k = 0; k < nE; k++) mix->selected_out[k] = 0;
}
// the selection of the call's final pass to the caller's host array
static int mix_selection_out(cgmr_ctx* ctx, const MixHost* M, int nE, const GnEdges& Ed) {
  if (!M || !Ed.mx.sel_out || nE <= 0) return 0;
  HIP_TRY(ctx, hipMemcpyAsync(M->mix->selected_out, Ed.mx.sel_out, 4 * (size_t)nE, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

// The arguments every *_optimize* entry point takes, checked alike; `name`: the entry point family in the error text
static int optimize_args_check(cgmr_ctx* ctx, const char* name, int nV, const double* poses, const uint8_t* fixed, int nE,
                               const int32_t* from_idx, const int32_t* to_idx, const double* meas, const double* info, int iters) {
  if (!ctx) return CGMR_E_INVALID;
  if (nV < 0 || nE < 0 || iters < 0 || (nV > 0 && (!poses || !fixed)) || (nE > 0 && (!from_idx || !to_idx || !meas || !info)))
    return set_err(ctx, CGMR_E_INVALID, "%s: null or negative argument", name);
  return 0;
}

// Around run(d_poses, Ed) -- gn_run, lm_run or dl_run on device arrays --: the robust description, and unless `dev` (poses,
// meas and info are the device's already) the host arrays staged through io_arena and the poses read back.  The poses and
// the robust statistics are returned when the call ended well, and with cholesky_too also on a Cholesky status.
template <typename Run>
static int optimize_staged(cgmr_ctx* ctx, const char* who, bool dev, bool cholesky_too, int nV, double* poses, int nE,
                           const double* meas, const double* info, const cgmr_robust* rk, const TypedHost* typed, Run&& run,
                           const MixHost* mix = nullptr) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  GnEdges Ed;
  int rc = robust_setup(ctx, rk, nE, dev, Ed, who);
  if (rc) return rc;
  rc = typed_upload(ctx, typed, Ed);
  if (rc) return rc;
  rc = mix_upload(ctx, mix, nE, Ed);
  if (rc) return rc;
  double* d_poses = poses;
  const size_t bp = sizeof(double) * 3 * (size_t)nV;
  if (dev) {
    Ed.meas_a = meas; Ed.info_a = info;
  } else {
    const size_t bm = sizeof(double) * 3 * (size_t)nE, bi = sizeof(double) * 6 * (size_t)nE;
    const size_t om = (bp + 255) & ~size_t(255), oi = (om + bm + 255) & ~size_t(255);
    rc = arena_reserve(ctx, ctx->io_arena, oi + bi + 256);
    if (rc) return rc;
    char* d = ctx->io_arena.ptr;
    HIP_TRY(ctx, hipMemcpyAsync(d, poses, bp, hipMemcpyHostToDevice, ctx->stream));
    if (Ed.mix) {                        // (a mixture pass reads the component lists alone: the first components stay on the host)
      Ed.meas_a = Ed.mx.cmeas; Ed.info_a = Ed.mx.cinfo;
    } else {
      HIP_TRY(ctx, hipMemcpyAsync(d + om, meas, bm, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(d + oi, info, bi, hipMemcpyHostToDevice, ctx->stream));
      Ed.meas_a = (const double*)(d + om); Ed.info_a = (const double*)(d + oi);
    }
    d_poses = (double*)d;
  }
  Ed.nA = nE; Ed.n_active = nE;
  rc = run(d_poses, Ed);
  if (rc == CGMR_OK || (cholesky_too && rc <= CGMR_E_CHOLESKY_BASE)) {
    if (!dev) {
      hipError_t e = hipMemcpyAsync(poses, d_poses, bp, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess) return set_err(ctx, CGMR_E_HIP, "pose read-back: %s", hipGetErrorString(e));
    }
    const int rs = robust_stats_out(ctx, rk, nE, Ed);
    if (rs) return rs;
    const int ms = mix_selection_out(ctx, mix, nE, Ed);
    if (ms) return ms;
  }
  return rc;
}

// What gn / lm / dl_optimize_impl do before they run, for `family` = "cgmr_gn_optimize", ...: the arguments, the factor types
// (F.typed), the mixture (F.mix; selected_out zeroed), and F.who, the name optimize_staged's own errors carry -- family +
// "_typed" for a typed call, else + plain / plain_dev.  The names are the ones these texts have always had.
struct OptimizeFront { TypedHost typed; MixHost mix; char who[64]; };
static int optimize_front(cgmr_ctx* ctx, const char* family, const char* plain, const char* plain_dev, int nV, const double* poses,
                          const uint8_t* fixed, int nE, const int32_t* from_idx, const int32_t* to_idx, const double* meas,
                          const double* info, int iters, bool dev, const cgmr_factor_types* ft, const cgmr_mixture* mix,
                          OptimizeFront& F) {
  int rc = optimize_args_check(ctx, family, nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters);
  if (rc) return rc;
  char name[64];
  snprintf(name, sizeof name, "%s%s", family, mix ? "_mixture" : dev ? "_typed_dev" : "_typed");
  rc = typed_check(ctx, name, ft, nV, nE, from_idx, to_idx, F.typed);
  if (rc) return rc;
  snprintf(name, sizeof name, "%s_mixture", family);
  rc = mix_check(ctx, name, mix, nE, F.typed, F.mix);
  if (rc) return rc;
  mix_selection_zero(mix, nE);
  snprintf(F.who, sizeof F.who, "%s%s", family, ft ? "_typed" : dev ? plain_dev : plain);
  return 0;
}

static int gn_optimize_impl(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                            const int32_t* to_idx, const double* meas, const double* info, int iters, double* chi2_out,
                            const cgmr_robust* rk, bool dev, const cgmr_factor_types* ft = nullptr,
                            const cgmr_mixture* mix = nullptr) {
  OptimizeFront F;
  int rc = optimize_front(ctx, "cgmr_gn_optimize", "_robust", "_robust_dev", nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, dev, ft, mix, F);
  if (rc) return rc;
  return optimize_staged(ctx, F.who, dev, true, nV, poses, nE, meas, info, rk, &F.typed,
                         [&](double* d_poses, const GnEdges& Ed) { return gn_run(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, Ed, iters, chi2_out); }, &F.mix);
}

static int lm_optimize_impl(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                            const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_lm_params* params,
                            double* chi2_out, double* lambda_out, int32_t* trials_out, int32_t* iters_done, const cgmr_robust* rk,
                            bool dev, const cgmr_factor_types* ft = nullptr, const cgmr_mixture* mix = nullptr) {
  OptimizeFront F;
  int rc = optimize_front(ctx, "cgmr_lm_optimize", "_robust", "_robust_dev", nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, dev, ft, mix, F);
  if (rc) return rc;
  return optimize_staged(ctx, F.who, dev, false, nV, poses, nE, meas, info, rk, &F.typed,
                         [&](double* d_poses, const GnEdges& Ed) {
                           return lm_run(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, Ed, iters, params, chi2_out, lambda_out, trials_out, iters_done);
                         }, &F.mix);
}

static int dl_optimize_impl(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                            const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_dl_params* params,
                            double* chi2_out, double* delta_out, int32_t* trials_out, int32_t* step_out, int32_t* iters_done,
                            const cgmr_robust* rk, bool dev, const cgmr_factor_types* ft = nullptr,
                            const cgmr_mixture* mix = nullptr) {
  OptimizeFront F;
  int rc = optimize_front(ctx, "cgmr_dl_optimize", "", "_dev", nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, dev, ft, mix, F);
  if (rc) return rc;
  if (!dl_params_ok(params))
    return set_err(ctx, CGMR_E_INVALID,
                   "cgmr_dl_optimize: max_trials must be >= 1, initial_delta / initial_lambda > 0, lambda_factor > 1, all finite");
  return optimize_staged(ctx, F.who, dev, true, nV, poses, nE, meas, info, rk, &F.typed,
                         [&](double* d_poses, const GnEdges& Ed) {
                           return dl_run(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, Ed, iters, params, chi2_out, delta_out, trials_out, step_out, iters_done);
                         }, &F.mix);
}


// ------------------------------------------------------------------------------------------------ graduated non-convexity
static cgmr_gnc_params gnc_defaults() {
  cgmr_gnc_params p;
  p.loss = CGMR_GNC_TLS; p.mu_factor = 1.4; p.max_outer = 100; p.inner_iters = 1; p.outer_per_wait = 8;
  p.barc_sq = nullptr; p.default_barc_sq = 0.0; p.known_inlier = nullptr; p.weight_out = nullptr; p.edge_chi2_out = nullptr;
  return p;
}

// gnc arena: state | mu, cost [max_outer + 1] | partial [max_outer + 1] || saved poses [3 nV] | weight, barc^2, r [nE] | the
// start's per-workgroup values | known mask [nE]
struct GncLayout {
  size_t o_mu, o_cost, o_part, rec_bytes, o_saved, o_w, o_c, o_r, o_wg, o_known, bytes;
  GncLayout(int max_outer, int nV, int nE) {
    BlobLayout B;
    B.add<GncState>(1);
    const size_t n = (size_t)max_outer + 1, e = (size_t)std::max(nE, 1);
    o_mu = B.add<double>(n); o_cost = B.add<double>(n); o_part = B.add<int32_t>(n);
    rec_bytes = B.off;
    o_saved = B.add<double>(3 * (size_t)std::max(nV, 1));
    o_w = B.add<double>(e); o_c = B.add<double>(e); o_r = B.add<double>(e); o_wg = B.add<double>((e + 255) / 256);
    o_known = B.add<uint8_t>(e);
    bytes = B.off + 256;
  }
};

// The third policy of tr_run.  A round: [the start: one chi-only pass for r, mu0;] up to outer_per_wait outer iterations.
struct GncPolicy {
  using State = GncState;
  static constexpr const char* kName = "graduated non-convexity";
  static constexpr bool kRunsEmpty = true;
  cgmr_gnc_params P;
  double *mu_out, *cost_out;
  int32_t *partial_out, *outer_done;
  GncDev L;
  GncLayout lay;
  int ran = 0;                                               // outer iterations run (finish())

  // (gnc_run has reserved the arena -- the per-edge arrays went up before the driver started -- and bound L)
  int reserve(cgmr_ctx*, int, int, int, int, size_t* rec_bytes) { *rec_bytes = lay.rec_bytes; return 0; }
  GncState start(int) const {
    GncState hs;
    hs.factor = P.mu_factor; hs.loss = P.loss; hs.max_outer = P.max_outer; hs.inner_iters = P.inner_iters;
    return hs;
  }
  GnEdges edges(const GnEdges& Ed, int mode, double* r_out) const {
    GnEdges E = Ed;
    E.gnc = true; E.ga = {L.weight, L.barc_sq, L.known, L.S, r_out, mode};
    return E;
  }
  static void outer_records(hipStream_t st, const GnDevice& D, void* self) { launch_gnc_outer(st, D, ((GncPolicy*)self)->L); }
  // One outer iteration, the same launches whatever happens (gnc_kernels.hip).  With nothing to move a pass is its
  // linearisation alone.
  void outer(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, int nV, double* d_poses, const GnEdges& Ed) {
    for (int i = 0; i < P.inner_iters; i++) {
      const GnEdges E = edges(Ed, i == 0 ? kGncCompute : kGncReuse, nullptr);
      if (D.nf > 0) {
        GnPassOpts o;
        if (i == 0) { o.after_assemble = outer_records; o.after_assemble_arg = this; }
        gn_pass_on(ctx, D, st, d_poses, E, o);
      } else if (i == 0) {
        launch_linearize(st, D, d_poses, E, 1);
        launch_gnc_outer(st, D, L);
      }
      launch_gnc_step(st, D, L, i + 1 == P.inner_iters);
    }
    launch_tr_commit(st, nV, d_poses, L.saved, &L.S->accept);
  }
  void queue_round(cgmr_ctx* ctx, GnDevice& D, hipStream_t st, int nV, double* d_poses, const GnEdges& Ed, const GncState& hs, int) {
    if (hs.need_init) {
      launch_linearize(st, D, d_poses, edges(Ed, kGncPlain, L.r), 1);
      launch_gnc_start(st, D, L);
    }
    const int n = std::min(P.outer_per_wait, P.max_outer - hs.iter);
    for (int t = 0; t < n; t++) outer(ctx, D, st, nV, d_poses, Ed);
  }
  GnCall::Readback also_read(const GnDevice&) { return {nullptr, nullptr, 0}; }
  void empty_system(GncState&, char*, double, int) const {}
  int finish(cgmr_ctx* ctx, const GncState& hs, const char* h, int ran_, int iters, int64_t waits) {
    ran = ran_;
    records_out(mu_out, (const double*)(h + lay.o_mu), ran, iters);
    records_out(partial_out, (const int32_t*)(h + lay.o_part), ran, iters);
    if (cost_out) for (int k = 0; k < ran; k++) cost_out[k] = ((const double*)(h + lay.o_cost))[k];   // (the rest: gnc_optimize_impl)
    if (outer_done) *outer_done = ran;
    ctx->gnc_stats[0] = waits;
    ctx->gnc_stats[1] = hs.inner_total;
    if (hs.failed)
      return set_err(ctx, CGMR_E_CHOLESKY_BASE - (hs.failed - 1),
                     "graduated non-convexity: Cholesky failed (non-positive pivot) in inner iteration %d; poses left at the last good update",
                     hs.failed - 1);
    return CGMR_OK;
  }
};

bool gnc_params_ok(const cgmr_gnc_params* params) {
  if (!params) return true;
  const cgmr_gnc_params& P = *params;
  return (P.loss == CGMR_GNC_TLS || P.loss == CGMR_GNC_GM) && std::isfinite(P.mu_factor) && P.mu_factor > 1 && P.max_outer >= 1 &&
         P.inner_iters >= 1 && P.outer_per_wait >= 1 && std::isfinite(P.default_barc_sq);
}
cgmr_gnc_params gnc_params_default() { return gnc_defaults(); }
double gnc_default_barc_sq(int dim) {
  const double quantile[4] = {0.0, 6.634896601021213, 9.21034037197618, 11.344866730144373};   // chi2 0.99, by dimension
  return quantile[dim < 1 ? 1 : dim > 3 ? 3 : dim];
}

// The driver of cgmr_gnc_optimize* and cgmr_graph_optimize_gnc: the arena, the per-edge arrays up, tr_run with GncPolicy, then
// the final statistics at the poses the call returns, with the weights of its last outer iteration.
int gnc_run(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et,
            const GnEdges& Ed, const cgmr_gnc_params& P, const double* barc_sq, const uint8_t* known, double* mu_out,
            double* cost_out, int32_t* partial_out, int32_t* outer_done, double* weight_out, double* edge_chi2_out,
            const int32_t* hub_vertices, int n_hub_vertices) {
  hipStream_t st = ctx->stream;
  GncPolicy pol{P, mu_out, cost_out, partial_out, outer_done, GncDev(), GncLayout(P.max_outer, nV, nE)};
  int r = arena_reserve(ctx, ctx->gnc_arena, pol.lay.bytes);
  if (r) return r;
  char* d = ctx->gnc_arena.ptr;
  GncDev& L = pol.L;
  L.S = (GncState*)d; L.rec_mu = (double*)(d + pol.lay.o_mu); L.rec_cost = (double*)(d + pol.lay.o_cost);
  L.rec_partial = (int32_t*)(d + pol.lay.o_part); L.saved = (double*)(d + pol.lay.o_saved); L.weight = (double*)(d + pol.lay.o_w);
  L.barc_sq = (double*)(d + pol.lay.o_c); L.r = (double*)(d + pol.lay.o_r); L.part = (double*)(d + pol.lay.o_wg);
  L.known = (uint8_t*)(d + pol.lay.o_known);
  if (nE > 0) {   // (pageable host memory: the copies have left the arrays when they return)
    HIP_TRY(ctx, hipMemcpyAsync(L.barc_sq, barc_sq, 8 * (size_t)nE, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(L.known, known, (size_t)nE, hipMemcpyHostToDevice, st));
  }
  r = tr_run(ctx, pol, nV, d_poses, fixed, nE, ef, et, Ed, P.max_outer, hub_vertices, n_hub_vertices);
  if (r != CGMR_OK && r > CGMR_E_CHOLESKY_BASE) return r;
  // the final statistics, at the poses the call returns and with the weights of its last outer iteration
  GnDevice& D = ctx->gn;
  double cost_end = 0.0;
  launch_linearize(st, D, d_poses, pol.edges(Ed, kGncReuse, L.r), 1);
  launch_chi2(st, D, D.chi2);
  HIP_TRY(ctx, hipMemcpyAsync(&cost_end, D.chi2, sizeof(double), hipMemcpyDeviceToHost, st));
  if (nE > 0 && weight_out) HIP_TRY(ctx, hipMemcpyAsync(weight_out, L.weight, 8 * (size_t)nE, hipMemcpyDeviceToHost, st));
  if (nE > 0 && edge_chi2_out) HIP_TRY(ctx, hipMemcpyAsync(edge_chi2_out, L.r, 8 * (size_t)nE, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (cost_out) for (int k = pol.ran; k <= P.max_outer; k++) cost_out[k] = cost_end;
  return r;
}

static int gnc_optimize_impl(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                             const int32_t* to_idx, const double* meas, const double* info, const cgmr_factor_types* ft,
                             const cgmr_gnc_params* params, double* mu_out, double* cost_out, int32_t* partial_out,
                             int32_t* outer_done, bool dev) {
  const char* who = dev ? "cgmr_gnc_optimize_dev" : "cgmr_gnc_optimize";
  int rc = optimize_args_check(ctx, who, nV, poses, fixed, nE, from_idx, to_idx, meas, info, 0);
  if (rc) return rc;
  const cgmr_gnc_params P = params ? *params : gnc_defaults();
  if (!gnc_params_ok(&P))
    return set_err(ctx, CGMR_E_INVALID, "%s: loss must be CGMR_GNC_TLS or CGMR_GNC_GM, mu_factor finite and > 1, max_outer / inner_iters / outer_per_wait >= 1, default_barc_sq finite", who);
  TypedHost typed;
  rc = typed_check(ctx, who, ft, nV, nE, from_idx, to_idx, typed);
  if (rc) return rc;
  std::vector<double> hc((size_t)nE);
  std::vector<uint8_t> hk((size_t)nE, 0);
  for (int k = 0; k < nE; k++) {
    hc[k] = P.barc_sq ? P.barc_sq[k] : P.default_barc_sq > 0 ? P.default_barc_sq : gnc_default_barc_sq(factor_dim(typed.any ? typed.ek[k] : CGMR_EDGE_SE2));
    if (!std::isfinite(hc[k]) || !(hc[k] > 0)) return set_err(ctx, CGMR_E_INVALID, "%s: barc_sq of edge %d must be finite and > 0", who, k);
    if (P.known_inlier) hk[k] = P.known_inlier[k] ? 1 : 0;
  }
  return optimize_staged(ctx, who, dev, true, nV, poses, nE, meas, info, nullptr, &typed, [&](double* d_poses, const GnEdges& Ed) {
    return gnc_run(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, Ed, P, hc.data(), hk.data(), mu_out, cost_out, partial_out, outer_done,
                   P.weight_out, P.edge_chi2_out);
  });
}

// cgmr_chordal_initialize*: the arguments checked, then which vertices each stage's terms touch -- a term whose information
// entries for the stage are all zero touches nothing -- from the host's copy of the information (a _dev call reads it back once)
static int chordal_impl(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                        const int32_t* to_idx, const double* meas, const double* info, const cgmr_factor_types* ft, int stages,
                        double* chi2_out, int32_t* counts_out, bool dev) {
  const char* who = ft ? (dev ? "cgmr_chordal_initialize_typed_dev" : "cgmr_chordal_initialize_typed")
                       : (dev ? "cgmr_chordal_initialize_dev" : "cgmr_chordal_initialize");
  int rc = optimize_args_check(ctx, who, nV, poses, fixed, nE, from_idx, to_idx, meas, info, 0);
  if (rc) return rc;
  if (stages < 1 || stages > 3) return set_err(ctx, CGMR_E_INVALID, "%s: stages must be 1 (rotation), 2 (translation) or 3 (both)", who);
  TypedHost typed;
  rc = typed_check(ctx, who, ft, nV, nE, from_idx, to_idx, typed);
  if (rc) return rc;
  for (int k = 0; k < nE; k++)
    if (from_idx[k] < 0 || from_idx[k] >= nV || to_idx[k] < 0 || to_idx[k] >= nV)
      return set_err(ctx, CGMR_E_INVALID, "%s: edge %d has a vertex index out of range", who, k);
  std::vector<double> hinfo;
  const double* hi = info;
  if (dev && nE > 0) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hinfo.resize(6 * (size_t)nE);
    HIP_TRY(ctx, hipMemcpyAsync(hinfo.data(), info, 48 * (size_t)nE, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    hi = hinfo.data();
  }
  std::vector<uint8_t> in_rot((size_t)nV, 0), in_tr((size_t)nV, 0);
  for (int k = 0; k < nE; k++) {
    const int dim = factor_dim(typed.any ? typed.ek[k] : CGMR_EDGE_SE2);      // 3: a heading term; 2 and 3: a position term
    const double* u = hi + 6 * (size_t)k;
    if (dim == 3 && u[5] != 0.0) in_rot[from_idx[k]] = in_rot[to_idx[k]] = 1;
    if (dim >= 2 && (u[0] != 0.0 || u[1] != 0.0 || u[3] != 0.0)) in_tr[from_idx[k]] = in_tr[to_idx[k]] = 1;
  }
  return optimize_staged(ctx, who, dev, true, nV, poses, nE, meas, info, nullptr, &typed, [&](double* d_poses, const GnEdges& Ed) {
    return chordal_run(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, Ed, stages, in_rot.data(), in_tr.data(), chi2_out, counts_out);
  });
}

}  // namespace cgmr

using namespace cgmr;

extern "C" {

int cgmr_version(void) { return 105; }   // 105: cgmr_*_optimize_robust*, cgmr_graph_set_edge_robust / _set_received_robust / _edge_stats added, later (same number: callers find them by their symbols) cgmr_marginals_robust, cgmr_marginals_all_robust, cgmr_covariance_estimate_robust, cgmr_condense_robust, cgmr_graph_set_condensed_robust, cgmr_dl_optimize*, cgmr_dl_last_stats, cgmr_graph_set_dogleg_params, cgmr_graph_dl_last (CGMR_ALG_DOGLEG), cgmr_marginals_joint, cgmr_marginals_pairs, cgmr_relative_covariance, cgmr_*_optimize_typed*, cgmr_marginals_typed, cgmr_marginals_all_typed, cgmr_marginals_joint_typed, cgmr_marginals_pairs_typed, cgmr_observation_covariance (and edge kind 2, CGMR_EDGE_BEARING_SE2_XY), cgmr_gnc_optimize*, cgmr_gnc_last_stats, cgmr_graph_set_edge_gnc / _set_received_gnc / _optimize_gnc / _gnc_weights / _keep_gnc_weights / _set_condensed_gnc; 104: cgmr_lm_optimize*, cgmr_lm_last_stats, cgmr_graph_set_algorithm / _lm_last added; 103: cgmr_marginals_all added; 102 (round 5): cgmr_match_last_redo_pairs / _path_counts, cgmr_graph_failed_batches, cgmr_comm_info added; nothing changed or removed

int cgmr_ctx_create(int device, void* hip_stream, cgmr_ctx** out) {
  if (!out) return CGMR_E_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return CGMR_E_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return CGMR_E_NO_DEVICE;
  cgmr_ctx* ctx = new cgmr_ctx();
  ctx->device = device;
  ctx->sw = read_switches();
  ctx->gn.sw = &ctx->sw;
  ctx->fwd_merge_any = ctx->sw.fwd_merge_any;
  if (hip_stream) { ctx->stream = (hipStream_t)hip_stream; ctx->own_stream = false; }
  else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return CGMR_E_HIP; }
    ctx->own_stream = true;
  }
  if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
      hipEventCreate(&ctx->ev_a) != hipSuccess || hipEventCreate(&ctx->ev_b) != hipSuccess) {
    cgmr_ctx_destroy(ctx);
    return CGMR_E_HIP;
  }
  *out = ctx;
  return CGMR_OK;
}

void cgmr_ctx_destroy(cgmr_ctx* ctx) {
  if (!ctx) return;
  // teardown: nothing useful can be done with a failing free, the statuses are dropped on purpose -- and a HIP runtime that
  // is already shutting down (a binding's garbage collector at interpreter exit) throws instead of returning an error
  try {
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->trace_n > 0)
    fprintf(stderr, "[gn] %lld solves: analysis + upload %.3f ms, masks %.3f ms, queueing the launches %.3f ms, waiting %.3f ms per solve\n", (long long)ctx->trace_n,
            1e3 * ctx->trace_sum[0] / ctx->trace_n, 1e3 * ctx->trace_sum[1] / ctx->trace_n, 1e3 * ctx->trace_sum[2] / ctx->trace_n, 1e3 * ctx->trace_sum[3] / ctx->trace_n);
  for (auto& q : ctx->graveyard) (void)hipFree(q.first);
  if (ctx->gn_arena.ptr) (void)hipFree(ctx->gn_arena.ptr);
  if (ctx->io_arena.ptr) (void)hipFree(ctx->io_arena.ptr);
  if (ctx->mt_arena.ptr) (void)hipFree(ctx->mt_arena.ptr);
  if (ctx->mtab_arena.ptr) (void)hipFree(ctx->mtab_arena.ptr);
  if (ctx->rep_arena.ptr) (void)hipFree(ctx->rep_arena.ptr);
  if (ctx->mg_arena.ptr) (void)hipFree(ctx->mg_arena.ptr);
  if (ctx->si_arena.ptr) (void)hipFree(ctx->si_arena.ptr);
  if (ctx->lm_arena.ptr) (void)hipFree(ctx->lm_arena.ptr);
  if (ctx->dl_arena.ptr) (void)hipFree(ctx->dl_arena.ptr);
  if (ctx->gnc_arena.ptr) (void)hipFree(ctx->gnc_arena.ptr);
  if (ctx->rk_arena.ptr) (void)hipFree(ctx->rk_arena.ptr);
  if (ctx->ty_arena.ptr) (void)hipFree(ctx->ty_arena.ptr);
  if (ctx->mix_arena.ptr) (void)hipFree(ctx->mix_arena.ptr);
  if (ctx->st_arena.ptr) (void)hipFree(ctx->st_arena.ptr);
  if (ctx->pinned_st) (void)hipHostFree(ctx->pinned_st);
  if (ctx->ev_st_copied) (void)hipEventDestroy(ctx->ev_st_copied);
  if (ctx->side) { (void)hipStreamSynchronize(ctx->side); (void)hipStreamDestroy(ctx->side); }
  for (hipEvent_t e : {ctx->side_fork, ctx->side_tail}) if (e) (void)hipEventDestroy(e);
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->pinned_mask) (void)hipHostFree(ctx->pinned_mask);
  for (hipEvent_t e : {ctx->ev0, ctx->ev1, ctx->ev_a, ctx->ev_b})
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  } catch (...) {
  }
  delete ctx;
}

const char* cgmr_last_error(const cgmr_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

void* cgmr_ctx_stream(const cgmr_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int cgmr_ctx_synchronize(cgmr_ctx* ctx) {
  if (!ctx) return CGMR_E_INVALID;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CGMR_OK;
}

int cgmr_gn_optimize_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE,
                         const int32_t* from_idx, const int32_t* to_idx, const double* d_meas,
                         const double* d_info, int iters, double* chi2_out) {
  return gn_optimize_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, iters, chi2_out, nullptr, true);
}

int cgmr_gn_optimize(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                     const int32_t* to_idx, const double* meas, const double* info, int iters, double* chi2_out) {
  return gn_optimize_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, chi2_out, nullptr, false);
}

int cgmr_lm_optimize_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                         const int32_t* to_idx, const double* d_meas, const double* d_info, int iters, const cgmr_lm_params* params,
                         double* chi2_out, double* lambda_out, int32_t* trials_out, int32_t* iters_done) {
  return lm_optimize_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, iters, params, chi2_out, lambda_out,
                          trials_out, iters_done, nullptr, true);
}

int cgmr_lm_optimize(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                     const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_lm_params* params,
                     double* chi2_out, double* lambda_out, int32_t* trials_out, int32_t* iters_done) {
  return lm_optimize_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, params, chi2_out, lambda_out, trials_out,
                          iters_done, nullptr, false);
}

int cgmr_gn_optimize_robust(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                            const int32_t* to_idx, const double* meas, const double* info, int iters, double* chi2_out,
                            const cgmr_robust* rk) {
  return gn_optimize_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, chi2_out, rk, false);
}

int cgmr_gn_optimize_robust_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                const int32_t* to_idx, const double* d_meas, const double* d_info, int iters, double* chi2_out,
                                const cgmr_robust* rk) {
  return gn_optimize_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, iters, chi2_out, rk, true);
}

int cgmr_lm_optimize_robust(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                            const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_lm_params* params,
                            double* chi2_out, double* lambda_out, int32_t* trials_out, int32_t* iters_done, const cgmr_robust* rk) {
  return lm_optimize_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, params, chi2_out, lambda_out, trials_out,
                          iters_done, rk, false);
}

int cgmr_lm_optimize_robust_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                const int32_t* to_idx, const double* d_meas, const double* d_info, int iters,
                                const cgmr_lm_params* params, double* chi2_out, double* lambda_out, int32_t* trials_out,
                                int32_t* iters_done, const cgmr_robust* rk) {
  return lm_optimize_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, iters, params, chi2_out, lambda_out,
                          trials_out, iters_done, rk, true);
}

int cgmr_lm_last_stats(const cgmr_ctx* ctx, int64_t out[2]) {
  if (!ctx || !out) return CGMR_E_INVALID;
  out[0] = ctx->lm_stats[0];
  out[1] = ctx->lm_stats[1];
  return CGMR_OK;
}

int cgmr_dl_optimize(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                     const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_dl_params* params,
                     double* chi2_out, double* delta_out, int32_t* trials_out, int32_t* step_out, int32_t* iters_done,
                     const cgmr_robust* rk) {
  return dl_optimize_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, params, chi2_out, delta_out, trials_out,
                          step_out, iters_done, rk, false);
}

int cgmr_dl_optimize_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                         const int32_t* to_idx, const double* d_meas, const double* d_info, int iters, const cgmr_dl_params* params,
                         double* chi2_out, double* delta_out, int32_t* trials_out, int32_t* step_out, int32_t* iters_done,
                         const cgmr_robust* rk) {
  return dl_optimize_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, iters, params, chi2_out, delta_out,
                          trials_out, step_out, iters_done, rk, true);
}

int cgmr_gn_optimize_typed(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                           const int32_t* to_idx, const double* meas, const double* info, int iters, double* chi2_out,
                           const cgmr_factor_types* types, const cgmr_robust* rk) {
  return gn_optimize_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, chi2_out, rk, false, types);
}

int cgmr_gn_optimize_typed_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                               const int32_t* to_idx, const double* d_meas, const double* d_info, int iters, double* chi2_out,
                               const cgmr_factor_types* types, const cgmr_robust* rk) {
  return gn_optimize_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, iters, chi2_out, rk, true, types);
}

int cgmr_lm_optimize_typed(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                           const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_lm_params* params,
                           double* chi2_out, double* lambda_out, int32_t* trials_out, int32_t* iters_done,
                           const cgmr_factor_types* types, const cgmr_robust* rk) {
  return lm_optimize_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, params, chi2_out, lambda_out, trials_out,
                          iters_done, rk, false, types);
}

int cgmr_lm_optimize_typed_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                               const int32_t* to_idx, const double* d_meas, const double* d_info, int iters,
                               const cgmr_lm_params* params, double* chi2_out, double* lambda_out, int32_t* trials_out,
                               int32_t* iters_done, const cgmr_factor_types* types, const cgmr_robust* rk) {
  return lm_optimize_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, iters, params, chi2_out, lambda_out,
                          trials_out, iters_done, rk, true, types);
}

int cgmr_dl_optimize_typed(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                           const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_dl_params* params,
                           double* chi2_out, double* delta_out, int32_t* trials_out, int32_t* step_out, int32_t* iters_done,
                           const cgmr_factor_types* types, const cgmr_robust* rk) {
  return dl_optimize_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, params, chi2_out, delta_out, trials_out,
                          step_out, iters_done, rk, false, types);
}

int cgmr_dl_optimize_typed_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                               const int32_t* to_idx, const double* d_meas, const double* d_info, int iters,
                               const cgmr_dl_params* params, double* chi2_out, double* delta_out, int32_t* trials_out,
                               int32_t* step_out, int32_t* iters_done, const cgmr_factor_types* types, const cgmr_robust* rk) {
  return dl_optimize_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, iters, params, chi2_out, delta_out,
                          trials_out, step_out, iters_done, rk, true, types);
}

int cgmr_marginals_typed(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                         const int32_t* et, const double* meas, const double* info, int nK, const int32_t* query,
                         double* cov_out, const cgmr_factor_types* types, const cgmr_robust* rk) {
  if (!ctx) return CGMR_E_INVALID;
  return marginal_driver(ctx, 0, nV, poses, fixed, nE, ef, et, meas, info, -1, nK, query, nullptr, nullptr, nullptr, cov_out, rk, types);
}

int cgmr_marginals_all_typed(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                             const int32_t* et, const double* meas, const double* info, double* cov_out, double* cross_out,
                             const cgmr_factor_types* types, const cgmr_robust* rk) {
  if (!ctx) return CGMR_E_INVALID;
  return marginals_all_driver(ctx, nV, poses, fixed, nE, ef, et, meas, info, cov_out, cross_out, rk, types);
}

/* max-mixture edges (include/cgmr.h: cgmr_mixture): the typed entry points without a robust kernel, plus the mixture */
int cgmr_gn_optimize_mixture(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                             const int32_t* to_idx, const double* meas, const double* info, int iters, double* chi2_out,
                             const cgmr_factor_types* ft, const cgmr_mixture* mix) {
  return gn_optimize_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, chi2_out, nullptr, false, ft, mix);
}
int cgmr_gn_optimize_mixture_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                 const int32_t* to_idx, const double* d_meas, const double* d_info, int iters, double* chi2_out,
                                 const cgmr_factor_types* ft, const cgmr_mixture* mix) {
  return gn_optimize_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, iters, chi2_out, nullptr, true, ft, mix);
}
int cgmr_lm_optimize_mixture(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                             const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_lm_params* params,
                             double* chi2_out, double* lambda_out, int32_t* trials_out, int32_t* iters_done,
                             const cgmr_factor_types* ft, const cgmr_mixture* mix) {
  return lm_optimize_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, params, chi2_out, lambda_out, trials_out,
                          iters_done, nullptr, false, ft, mix);
}
int cgmr_lm_optimize_mixture_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                 const int32_t* to_idx, const double* d_meas, const double* d_info, int iters,
                                 const cgmr_lm_params* params, double* chi2_out, double* lambda_out, int32_t* trials_out,
                                 int32_t* iters_done, const cgmr_factor_types* ft, const cgmr_mixture* mix) {
  return lm_optimize_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, iters, params, chi2_out, lambda_out,
                          trials_out, iters_done, nullptr, true, ft, mix);
}
int cgmr_dl_optimize_mixture(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                             const int32_t* to_idx, const double* meas, const double* info, int iters, const cgmr_dl_params* params,
                             double* chi2_out, double* delta_out, int32_t* trials_out, int32_t* step_out, int32_t* iters_done,
                             const cgmr_factor_types* ft, const cgmr_mixture* mix) {
  return dl_optimize_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, iters, params, chi2_out, delta_out, trials_out,
                          step_out, iters_done, nullptr, false, ft, mix);
}
int cgmr_dl_optimize_mixture_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                 const int32_t* to_idx, const double* d_meas, const double* d_info, int iters,
                                 const cgmr_dl_params* params, double* chi2_out, double* delta_out, int32_t* trials_out,
                                 int32_t* step_out, int32_t* iters_done, const cgmr_factor_types* ft, const cgmr_mixture* mix) {
  return dl_optimize_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, iters, params, chi2_out, delta_out,
                          trials_out, step_out, iters_done, nullptr, true, ft, mix);
}
/* chi2 and selection at the given poses: Gauss-Newton with no iteration, which is its one chi-only pass */
int cgmr_mixture_select(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                        const int32_t* to_idx, const double* meas, const double* info, const cgmr_factor_types* ft,
                        const cgmr_mixture* mix, double* chi2_out) {
  if (!ctx) return CGMR_E_INVALID;
  if (nV < 0 || (nV > 0 && !poses)) return set_err(ctx, CGMR_E_INVALID, "cgmr_mixture_select: null or negative argument");
  std::vector<double> x(poses, poses + 3 * (size_t)nV);
  return gn_optimize_impl(ctx, nV, x.data(), fixed, nE, from_idx, to_idx, meas, info, 0, chi2_out, nullptr, false, ft, mix);
}

cgmr_gnc_params cgmr_gnc_params_default(void) { return gnc_defaults(); }

int cgmr_gnc_optimize(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                      const int32_t* to_idx, const double* meas, const double* info, const cgmr_factor_types* types,
                      const cgmr_gnc_params* params, double* mu_out, double* cost_out, int32_t* partial_out, int32_t* outer_done) {
  return gnc_optimize_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, types, params, mu_out, cost_out, partial_out,
                           outer_done, false);
}

int cgmr_gnc_optimize_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                          const int32_t* to_idx, const double* d_meas, const double* d_info, const cgmr_factor_types* types,
                          const cgmr_gnc_params* params, double* mu_out, double* cost_out, int32_t* partial_out,
                          int32_t* outer_done) {
  return gnc_optimize_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, types, params, mu_out, cost_out,
                           partial_out, outer_done, true);
}

int cgmr_chordal_initialize(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                            const int32_t* to_idx, const double* meas, const double* info, int stages, double* chi2_out,
                            int32_t* counts_out) {
  return chordal_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, nullptr, stages, chi2_out, counts_out, false);
}

int cgmr_chordal_initialize_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                const int32_t* to_idx, const double* d_meas, const double* d_info, int stages, double* chi2_out,
                                int32_t* counts_out) {
  return chordal_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, nullptr, stages, chi2_out, counts_out, true);
}

int cgmr_chordal_initialize_typed(cgmr_ctx* ctx, int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx,
                                  const int32_t* to_idx, const double* meas, const double* info, int stages, double* chi2_out,
                                  int32_t* counts_out, const cgmr_factor_types* types) {
  return chordal_impl(ctx, nV, poses, fixed, nE, from_idx, to_idx, meas, info, types, stages, chi2_out, counts_out, false);
}

int cgmr_chordal_initialize_typed_dev(cgmr_ctx* ctx, int nV, double* d_poses, const uint8_t* fixed, int nE,
                                      const int32_t* from_idx, const int32_t* to_idx, const double* d_meas, const double* d_info,
                                      int stages, double* chi2_out, int32_t* counts_out, const cgmr_factor_types* types) {
  return chordal_impl(ctx, nV, d_poses, fixed, nE, from_idx, to_idx, d_meas, d_info, types, stages, chi2_out, counts_out, true);
}

int cgmr_initial_guess(int nV, double* poses, const uint8_t* fixed, int nE, const int32_t* from_idx, const int32_t* to_idx,
                       const double* meas) {
  if (nV < 0 || nE < 0 || (nV > 0 && (!poses || !fixed)) || (nE > 0 && (!from_idx || !to_idx || !meas))) return CGMR_E_INVALID;
  for (int k = 0; k < nE; k++)
    if (from_idx[k] < 0 || from_idx[k] >= nV || to_idx[k] < 0 || to_idx[k] >= nV) return CGMR_E_INVALID;
  initial_guess_host(nV, poses, fixed, nE, from_idx, to_idx, meas);
  return CGMR_OK;
}

int cgmr_gnc_last_stats(const cgmr_ctx* ctx, int64_t out[2]) {
  if (!ctx || !out) return CGMR_E_INVALID;
  out[0] = ctx->gnc_stats[0];
  out[1] = ctx->gnc_stats[1];
  return CGMR_OK;
}

int cgmr_dl_last_stats(const cgmr_ctx* ctx, int64_t out[3]) {
  if (!ctx || !out) return CGMR_E_INVALID;
  for (int k = 0; k < 3; k++) out[k] = ctx->dl_stats[k];
  return CGMR_OK;
}

static void symbolic_info_out(const Symbolic& S, int nV, int64_t out[16], int32_t* perm_out) {
  out[0] = S.nf; out[1] = S.nb; out[2] = (int64_t)S.fronts.size(); out[3] = (int64_t)S.level_ptr.size() - 1;
  out[4] = S.L_doubles; out[5] = S.U_doubles; out[6] = S.max_ns; out[7] = (int64_t)S.flops;
  out[8] = (int64_t)(1e6 * S.t_order); out[9] = (int64_t)(1e6 * S.t_struct);
  out[10] = out[11] = out[12] = 0;
  out[13] = (int64_t)S.gn_level_ptr.size() - 1; out[14] = (int64_t)S.top_fronts.size(); out[15] = 3 * (int64_t)S.top_nposes;
  for (const FrontDesc& F : S.fronts) {
    out[12] += pan_size(F.ns) * F.pan_slots;
    out[10] = std::max<int64_t>(out[10], F.nchild);
    if (F.ns >= 1 && F.ns <= 32) out[11] = std::max<int64_t>(out[11], F.nchild);
  }
  if (perm_out) memcpy(perm_out, S.vperm.data(), sizeof(int32_t) * nV);
}

int cgmr_gn_symbolic_info(int nV, const uint8_t* fixed, int nE, const int32_t* from_idx, const int32_t* to_idx,
                          int64_t out[16], int32_t* perm_out) {
  if (nV < 0 || nE < 0 || !out) return CGMR_E_INVALID;
  Symbolic S;
  (void)fixed;          // the solver applies the fixed flags numerically: they are not part of the analysis
  int rc = analyze(nV, nullptr, nE, from_idx, to_idx, S, read_switches());
  if (rc) return CGMR_E_INVALID;
  symbolic_info_out(S, nV, out, perm_out);
  return CGMR_OK;
}

int cgmr_gn_symbolic_info_grown(int nV0, int nE0, int n_steps, const int32_t* nV_step, const int32_t* nE_step,
                                const int32_t* from_idx, const int32_t* to_idx, int64_t out[16], int32_t* perm_out,
                                int32_t* n_extended_out) {
  if (nV0 < 0 || nE0 < 0 || n_steps < 0 || !out || (n_steps > 0 && (!nV_step || !nE_step))) return CGMR_E_INVALID;
  Symbolic S;
  const Switches sw = read_switches();
  if (analyze(nV0, nullptr, nE0, from_idx, to_idx, S, sw)) return CGMR_E_INVALID;
  int nV = nV0, next = 0;
  for (int k = 0; k < n_steps; k++) {
    if (nV_step[k] < nV || nE_step[k] < S.nE) return CGMR_E_INVALID;
    Symbolic old = std::move(S);
    if (analyze(nV_step[k], nullptr, nE_step[k], from_idx, to_idx, S, sw, &old)) return CGMR_E_INVALID;
    nV = nV_step[k];
    next += S.extended ? 1 : 0;
  }
  if (n_extended_out) *n_extended_out = next;
  symbolic_info_out(S, nV, out, perm_out);
  return CGMR_OK;
}

int cgmr_marginals(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                   const int32_t* et, const double* meas, const double* info, int nK, const int32_t* query,
                   double* cov_out) {
  if (!ctx || !cov_out) return CGMR_E_INVALID;
  return marginal_driver(ctx, 0, nV, poses, fixed, nE, ef, et, meas, info, -1, nK, query, nullptr, nullptr, nullptr, cov_out, nullptr);
}

int cgmr_marginals_all(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                       const int32_t* et, const double* meas, const double* info, double* cov_out, double* cross_out) {
  if (!ctx) return CGMR_E_INVALID;
  return marginals_all_driver(ctx, nV, poses, fixed, nE, ef, et, meas, info, cov_out, cross_out, nullptr);
}

int cgmr_covariance_estimate(cgmr_ctx* ctx, int nV, const double* poses, int nE, const int32_t* ef, const int32_t* et,
                             const double* meas, const double* info, int gauge, int nK, const int32_t* query,
                             double* cov_out) {
  if (!ctx || !cov_out) return CGMR_E_INVALID;
  return marginal_driver(ctx, 1, nV, poses, nullptr, nE, ef, et, meas, info, gauge, nK, query, nullptr, nullptr, nullptr, cov_out,
                         nullptr);
}

int cgmr_condense(cgmr_ctx* ctx, int nV, const double* poses, int nE, const int32_t* ef, const int32_t* et,
                  const double* meas, const double* info, int gauge, int nK, const int32_t* query, int32_t* to_out,
                  double* est_out, double* info_out, double* cov_out) {
  if (!ctx || !to_out || !est_out || !info_out) return CGMR_E_INVALID;
  return marginal_driver(ctx, 2, nV, poses, nullptr, nE, ef, et, meas, info, gauge, nK, query, to_out, est_out, info_out, cov_out,
                         nullptr);
}

int cgmr_marginals_robust(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                          const int32_t* et, const double* meas, const double* info, int nK, const int32_t* query,
                          double* cov_out, const cgmr_robust* rk) {
  if (!ctx || !cov_out) return CGMR_E_INVALID;
  return marginal_driver(ctx, 0, nV, poses, fixed, nE, ef, et, meas, info, -1, nK, query, nullptr, nullptr, nullptr, cov_out, rk);
}

int cgmr_marginals_all_robust(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                              const int32_t* et, const double* meas, const double* info, double* cov_out, double* cross_out,
                              const cgmr_robust* rk) {
  if (!ctx) return CGMR_E_INVALID;
  return marginals_all_driver(ctx, nV, poses, fixed, nE, ef, et, meas, info, cov_out, cross_out, rk);
}

int cgmr_covariance_estimate_robust(cgmr_ctx* ctx, int nV, const double* poses, int nE, const int32_t* ef, const int32_t* et,
                                    const double* meas, const double* info, int gauge, int nK, const int32_t* query,
                                    double* cov_out, const cgmr_robust* rk) {
  if (!ctx || !cov_out) return CGMR_E_INVALID;
  return marginal_driver(ctx, 1, nV, poses, nullptr, nE, ef, et, meas, info, gauge, nK, query, nullptr, nullptr, nullptr, cov_out, rk);
}

int cgmr_condense_robust(cgmr_ctx* ctx, int nV, const double* poses, int nE, const int32_t* ef, const int32_t* et,
                         const double* meas, const double* info, int gauge, int nK, const int32_t* query, int32_t* to_out,
                         double* est_out, double* info_out, double* cov_out, const cgmr_robust* rk) {
  if (!ctx || !to_out || !est_out || !info_out) return CGMR_E_INVALID;
  return marginal_driver(ctx, 2, nV, poses, nullptr, nE, ef, et, meas, info, gauge, nK, query, to_out, est_out, info_out, cov_out, rk);
}

int cgmr_marginals_joint(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                         const int32_t* et, const double* meas, const double* info, int nK, const int32_t* query, double* cov_out,
                         const cgmr_robust* rk) {
  if (!ctx) return CGMR_E_INVALID;
  return joint_driver(ctx, "cgmr_marginals_joint", 0, nV, poses, fixed, nE, ef, et, meas, info, nK, query, nullptr, cov_out, nullptr, nullptr, nullptr, nullptr, rk);
}

int cgmr_marginals_pairs(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                         const int32_t* et, const double* meas, const double* info, int nP, const int32_t* pair_a,
                         const int32_t* pair_b, double* cov_aa_out, double* cov_ab_out, double* cov_bb_out, const cgmr_robust* rk) {
  if (!ctx) return CGMR_E_INVALID;
  return joint_driver(ctx, "cgmr_marginals_pairs", 1, nV, poses, fixed, nE, ef, et, meas, info, nP, pair_a, pair_b, cov_aa_out, cov_ab_out, cov_bb_out, nullptr,
                      nullptr, rk);
}

int cgmr_relative_covariance(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                             const int32_t* et, const double* meas, const double* info, int nP, const int32_t* pair_a,
                             const int32_t* pair_b, double* rel_xyt_out, double* rel_cov_out, const double* hyp_meas,
                             const double* hyp_info, double* d2_out, const cgmr_robust* rk) {
  if (!ctx) return CGMR_E_INVALID;
  return joint_driver(ctx, "cgmr_relative_covariance", 2, nV, poses, fixed, nE, ef, et, meas, info, nP, pair_a, pair_b, rel_xyt_out, rel_cov_out, d2_out, hyp_meas,
                      hyp_info, rk);
}

int cgmr_marginals_joint_typed(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                               const int32_t* et, const double* meas, const double* info, int nK, const int32_t* query,
                               double* cov_out, const cgmr_factor_types* types, const cgmr_robust* rk) {
  if (!ctx) return CGMR_E_INVALID;
  return joint_driver(ctx, "cgmr_marginals_joint_typed", 0, nV, poses, fixed, nE, ef, et, meas, info, nK, query, nullptr, cov_out, nullptr,
                      nullptr, nullptr, nullptr, rk, types);
}

int cgmr_marginals_pairs_typed(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                               const int32_t* et, const double* meas, const double* info, int nP, const int32_t* pair_a,
                               const int32_t* pair_b, double* cov_aa_out, double* cov_ab_out, double* cov_bb_out,
                               const cgmr_factor_types* types, const cgmr_robust* rk) {
  if (!ctx) return CGMR_E_INVALID;
  return joint_driver(ctx, "cgmr_marginals_pairs_typed", 1, nV, poses, fixed, nE, ef, et, meas, info, nP, pair_a, pair_b, cov_aa_out,
                      cov_ab_out, cov_bb_out, nullptr, nullptr, rk, types);
}

int cgmr_observation_covariance(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                                const int32_t* et, const double* meas, const double* info, int nP, const int32_t* pair_a,
                                const int32_t* pair_b, const uint8_t* obs_kind, double* z_out, double* cov_out,
                                const double* hyp_meas, const double* hyp_info, double* d2_out, const cgmr_factor_types* types,
                                const cgmr_robust* rk) {
  if (!ctx) return CGMR_E_INVALID;
  return joint_driver(ctx, "cgmr_observation_covariance", 2, nV, poses, fixed, nE, ef, et, meas, info, nP, pair_a, pair_b, z_out, cov_out,
                      d2_out, hyp_meas, hyp_info, rk, types, true, obs_kind);
}

int cgmr_closure_consistency(cgmr_ctx* ctx, int nV, const double* poses, const uint8_t* fixed, int nE, const int32_t* ef,
                             const int32_t* et, const double* meas, const double* info, int nC, const int32_t* cl_a,
                             const int32_t* cl_b, const double* cl_meas, const double* cl_info, double gamma, double* d2_out,
                             uint64_t* adj_out, int32_t* clique_out, int32_t* clique_size_out, int32_t* seed_out,
                             const cgmr_robust* rk) {
  if (!ctx) return CGMR_E_INVALID;
  return pcm_driver(ctx, nV, poses, fixed, nE, ef, et, meas, info, nC, cl_a, cl_b, cl_meas, cl_info, gamma, d2_out, adj_out, clique_out,
                    clique_size_out, seed_out, rk);
}

int cgmr_max_clique_greedy(cgmr_ctx* ctx, int n, const uint64_t* adj_bits, int32_t* clique_out, int32_t* clique_size_out,
                           int32_t* seed_out) {
  if (!ctx) return CGMR_E_INVALID;
  return clique_driver(ctx, n, adj_bits, clique_out, clique_size_out, seed_out);
}

int cgmr_set_symbolic_cache(cgmr_ctx* ctx, int on) {
  if (!ctx) return CGMR_E_INVALID;
  ctx->sym_cache_on = on != 0;
  ctx->sym_valid = false;
  return CGMR_OK;
}

}  // extern "C"
namespace cgmr {
// gn_symbolic.cpp: the helper pool as it runs -- threads an analysis uses (caller included), 1 if the helpers are pinned around
// a last-level cache, the caller's home CPU while it analyses (-1: not pinned), CPUs the process may use, moves of the pool
void host_pool_info(int out[5]);
}
extern "C" {

int cgmr_host_threads_info(int32_t out[5]) {
  if (!out) return CGMR_E_INVALID;
  int v[5];
  host_pool_info(v);
  for (int k = 0; k < 5; k++) out[k] = v[k];
  return CGMR_OK;
}

int cgmr_symbolic_cache_stats(const cgmr_ctx* ctx, int64_t out[2]) {     // the two-value ABI of version 100
  if (!ctx || !out) return CGMR_E_INVALID;
  out[0] = ctx->sym_hits; out[1] = ctx->sym_misses + ctx->sym_extended;
  return CGMR_OK;
}

int cgmr_symbolic_cache_stats3(const cgmr_ctx* ctx, int64_t out[3]) {
  if (!ctx || !out) return CGMR_E_INVALID;
  out[0] = ctx->sym_hits; out[1] = ctx->sym_misses; out[2] = ctx->sym_extended;
  return CGMR_OK;
}

int64_t cgmr_gn_timeouts(const cgmr_ctx* ctx) { return ctx ? ctx->gn_timeouts : -1; }

int cgmr_switches(const cgmr_ctx* ctx, char* buf, int cap) {
  if (cap < 0 || (cap > 0 && !buf)) return CGMR_E_INVALID;
  const Switches defaults;
  return list_switches(ctx ? ctx->sw : defaults, ctx ? process_switches() : defaults, buf, cap);
}

int cgmr_gn_last_timing(const cgmr_ctx* ctx, double out[5]) {
  if (!ctx || !out) return CGMR_E_INVALID;
  memcpy(out, ctx->timing, sizeof(double) * 5);
  return CGMR_OK;
}

int cgmr_set_profiling(cgmr_ctx* ctx, int on) {
  if (!ctx) return CGMR_E_INVALID;
  ctx->profiling = on != 0;
  memset(ctx->ksec, 0, sizeof ctx->ksec);
  memset(ctx->klaunch, 0, sizeof ctx->klaunch);
  ctx->ev_cls.clear();
  if (on && ctx->ev_pool.empty()) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->ev_pool.resize(2 * 2048);              // enough for optimize(~30) on a 21-level tree; further launches go untimed
    for (hipEvent_t& e : ctx->ev_pool)
      if (hipEventCreate(&e) != hipSuccess) { ctx->ev_pool.clear(); return set_err(ctx, CGMR_E_HIP, "hipEventCreate failed"); }
  }
  return CGMR_OK;
}

int cgmr_gn_kernel_times(const cgmr_ctx* ctx, double seconds_out[8], int64_t launches_out[8]) {
  if (!ctx || !seconds_out || !launches_out) return CGMR_E_INVALID;
  memcpy(seconds_out, ctx->ksec, sizeof(double) * 8);
  memcpy(launches_out, ctx->klaunch, sizeof(int64_t) * 8);
  return CGMR_OK;
}

// the same with the classes beyond the first eight: 8 = front_level (k_front_level: a tree level's factorisation and its update
// tiles in one launch); classes 9..11 are pcm_driver's / clique_driver's
extern "C" int cgmr_gn_kernel_times_ex(const cgmr_ctx* ctx, double seconds_out[12], int64_t launches_out[12]) {
  if (!ctx || !seconds_out || !launches_out) return CGMR_E_INVALID;
  memcpy(seconds_out, ctx->ksec, sizeof(double) * 12);
  memcpy(launches_out, ctx->klaunch, sizeof(int64_t) * 12);
  return CGMR_OK;
}

}  // extern "C"

// Debugging aid (host only): the front table of a graph's symbolic analysis, 6 ints per front: c0, nc, ns, parent, level, nchild.
extern "C" int cgmr_debug_fronts(int nV, const uint8_t* fixed, int nE, const int32_t* ef, const int32_t* et, int cap, int32_t* out) {
  Symbolic S;
  (void)fixed;
  if (analyze(nV, nullptr, nE, ef, et, S, read_switches())) return -1;
  int n = (int)S.fronts.size();
  for (int f = 0; f < n && f < cap; f++) {
    const FrontDesc& F = S.fronts[f];
    int32_t* o = out + 6 * f;
    o[0] = F.c0; o[1] = F.nc; o[2] = F.ns; o[3] = F.parent; o[4] = F.level; o[5] = F.nchild;
  }
  return n;
}

// The children's schedule of every front (tests): out[4 f ..] = sched_t, sched_slot, pan_slots, 1 if the front adds into its
// parent's panel (0: root, or child of the top block)
extern "C" int cgmr_debug_schedule(int nV, int nE, const int32_t* ef, const int32_t* et, int cap, int32_t* out) {
  Symbolic S;
  if (analyze(nV, nullptr, nE, ef, et, S, read_switches())) return -1;
  int n = (int)S.fronts.size();
  for (int f = 0; f < n && f < cap; f++) {
    const FrontDesc& F = S.fronts[f];
    int32_t* o = out + 4 * f;
    o[0] = F.sched_t; o[1] = F.sched_slot; o[2] = F.pan_slots; o[3] = F.ppan_off >= 0 ? 1 : 0;
  }
  return n;
}

// Debugging aid: the (front, chunk) of every work item of the last analysed graph, and each front's parent / level.
extern "C" int cgmr_debug_worklist(const cgmr_ctx* ctx, int32_t* front_out, int32_t* chunk_out, int cap, int32_t* parent_out,
                                   int32_t* level_out, int32_t* ns_out, int fcap) {
  if (!ctx) return -1;
  const Symbolic& S = ctx->sym;
  int n = 0;
  for (int l = 0; l + 1 < (int)S.level_ptr.size(); l++)
    for (int q = S.level_ptr[l]; q < S.level_ptr[l + 1]; q++) {
      int f = S.level_fronts[q];
      int r = 3 * S.fronts[f].ns;
      const int chunk_rows = l < (int)ctx->gn.h_level_chunk.size() ? ctx->gn.h_level_chunk[l] : kChunkRows;
      int nchunk = std::max(1, (r + chunk_rows - 1) / chunk_rows);
      for (int c = 0; c < nchunk; c++) { if (n < cap) { front_out[n] = f; chunk_out[n] = c; } n++; }
    }
  for (int f = 0; f < (int)S.fronts.size() && f < fcap; f++) { parent_out[f] = S.fronts[f].parent; level_out[f] = S.fronts[f].level; ns_out[f] = S.fronts[f].ns; }
  return n;
}

// Host-only test hook: a sequence of complete edge lists analysed one after the other the way a context with the analysis
// cache on does (step k: vertices nV[k], edges e_ptr[k] .. e_ptr[k+1] of ef / et, hub hints h_ptr[k] .. h_ptr[k+1] of hubs).
// out / perm_out / fronts_out (6 ints per front as cgmr_debug_fronts) describe the last analysis; returns its front count.
extern "C" int cgmr_debug_symbolic_steps(int n_steps, const int32_t* nV, const int32_t* e_ptr, const int32_t* ef, const int32_t* et,
                                         const int32_t* h_ptr, const int32_t* hubs, int64_t out[16], int32_t* perm_out,
                                         int32_t* n_extended_out, int fcap, int32_t* fronts_out, int64_t* per_step_out) {
  if (n_steps < 1 || !nV || !e_ptr || !out) return -1;
  Symbolic S;
  const Switches sw = read_switches();
  std::vector<int32_t> pef, pet;
  int prev_nV = 0, next = 0;
  for (int k = 0; k < n_steps; k++) {
    const int nE = e_ptr[k + 1] - e_ptr[k];
    const int nh = h_ptr ? h_ptr[k + 1] - h_ptr[k] : 0;
    if (analyze_next(S, sw, k > 0, prev_nV, pef, pet, nV[k], nE, ef + e_ptr[k], et + e_ptr[k], nh ? hubs + h_ptr[k] : nullptr, nh)) return -1;
    if (k > 0 && S.extended) next++;
    if (per_step_out) {                                     // per step: levels, extended, ordering us, structure us, factor flops
      int64_t* o = per_step_out + 5 * (size_t)k;
      o[0] = (int64_t)S.level_ptr.size() - 1; o[1] = S.extended ? 1 : 0; o[2] = (int64_t)(1e6 * S.t_order); o[3] = (int64_t)(1e6 * S.t_struct); o[4] = (int64_t)S.flops;
    }
    pef.assign(ef + e_ptr[k], ef + e_ptr[k + 1]);
    pet.assign(et + e_ptr[k], et + e_ptr[k + 1]);
    prev_nV = nV[k];
  }
  if (n_extended_out) *n_extended_out = next;
  symbolic_info_out(S, nV[n_steps - 1], out, perm_out);
  const int n = (int)S.fronts.size();
  for (int f = 0; f < n && f < fcap && fronts_out; f++) {
    const FrontDesc& F = S.fronts[f];
    int32_t* o = fronts_out + 6 * f;
    o[0] = F.c0; o[1] = F.nc; o[2] = F.ns; o[3] = F.parent; o[4] = F.level; o[5] = F.nchild;
  }
  return n;
}

// Tests: the assembly lists (gn_symbolic.h: asm_ptr / asm_src) as the host's reference builds them for an edge list (ctx ==
// nullptr: structure_reference), or as they stand on the device for the graph the context analysed last (ef / et ignored).  Returns nf + nb (the number of
// keys; -1: error), the number of list entries in *n_src_out.
extern "C" int cgmr_debug_asm_lists(cgmr_ctx* ctx, int nV, int nE, const int32_t* ef, const int32_t* et, int cap_ptr, int32_t* ptr_out,
                                    int cap_src, int32_t* src_out, int32_t* n_src_out) {
  if (!ptr_out || !src_out || !n_src_out) return -1;
  if (!ctx) {
    Symbolic S;
    StructureRef R;
    if (analyze(nV, nullptr, nE, ef, et, S, read_switches()) || structure_reference(S, nE, ef, et, R)) return -1;
    const int nk = S.nf + S.nb;
    if (nk + 1 > cap_ptr || (int)R.asm_src.size() > cap_src) return -1;
    if (R.asm_ptr.empty()) { *n_src_out = 0; return nk; }
    memcpy(ptr_out, R.asm_ptr.data(), 4 * (size_t)(nk + 1));
    memcpy(src_out, R.asm_src.data(), 4 * R.asm_src.size());
    *n_src_out = (int)R.asm_src.size();
    return nk;
  }
  const GnDevice& D = ctx->gn;
  const int nk = D.nf + D.nb;
  if (nk + 1 > cap_ptr || !D.asm_ptr) return -1;
  if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
  if (hipMemcpy(ptr_out, D.asm_ptr, 4 * (size_t)(nk + 1), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  const int ns = ptr_out[nk];
  if (ns > cap_src) return -1;
  if (ns > 0 && hipMemcpy(src_out, D.asm_src, 4 * (size_t)ns, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  *n_src_out = ns;
  return nk;
}

// Tests: rel | inv | blk_dst | b_dst (gn_symbolic.h) one behind the other, as the host's reference builds them for an edge list
// (ctx == nullptr: structure_reference) or as they stand on the device for the graph the context analysed last.  Returns the number of ints, -1: error.
extern "C" int cgmr_debug_maps(cgmr_ctx* ctx, int nV, int nE, const int32_t* ef, const int32_t* et, int cap, int32_t* out) {
  if (!out) return -1;
  if (!ctx) {
    Symbolic S;
    StructureRef R;
    if (analyze(nV, nullptr, nE, ef, et, S, read_switches()) || structure_reference(S, nE, ef, et, R)) return -1;
    const size_t n = R.rel.size() + R.inv.size() + R.blk_dst.size() + R.b_dst.size();
    if (n > (size_t)cap) return -1;
    int32_t* o = out;
    for (const std::vector<int32_t>* v : {&R.rel, &R.inv, &R.blk_dst, &R.b_dst}) { memcpy(o, v->data(), 4 * v->size()); o += v->size(); }
    return (int)n;
  }
  const GnDevice& D = ctx->gn;
  const Symbolic& S = ctx->sym;
  const size_t sizes[4] = {(size_t)S.n_rel, (size_t)S.n_inv, (size_t)S.nf + S.nb, (size_t)S.nf};
  const int32_t* srcs[4] = {D.rel, D.inv, D.blk_dst, D.b_dst};
  if (sizes[0] + sizes[1] + sizes[2] + sizes[3] > (size_t)cap) return -1;
  if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
  int32_t* o = out;
  for (int k = 0; k < 4; k++) {
    if (sizes[k] && hipMemcpy(o, srcs[k], 4 * sizes[k], hipMemcpyDeviceToHost) != hipSuccess) return -1;
    o += sizes[k];
  }
  return (int)(o - out);
}

// Tests: the factor kernel's work records (gn_symbolic.h: WorkRec) of the graph the context analysed last, as they stand on the
// device (dev_out) and as a host loop over the context's analysis and chunk lengths writes them (ref_out); cap records each.
// Returns the number of records (more than cap: nothing was written), -1: error.
extern "C" int cgmr_debug_work_records(cgmr_ctx* ctx, int cap, void* dev_out, void* ref_out) {
  if (!ctx) return -1;
  const GnDevice& D = ctx->gn;
  const Symbolic& S = ctx->sym;
  const int n_work = D.h_work_ptr.empty() ? 0 : D.h_work_ptr.back();
  if (n_work > cap || n_work == 0) return n_work;
  if (!dev_out || !ref_out) return -1;
  if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
  if (n_work && hipMemcpy(dev_out, D.work, sizeof(WorkRec) * (size_t)n_work, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  WorkRec* work = static_cast<WorkRec*>(ref_out);
  for (int l = 0; l < D.nlevels; l++) {
    const int chunk_rows = D.h_level_chunk[l];
    int w = D.h_work_ptr[l];
    for (int q = S.gn_level_ptr[l]; q < S.gn_level_ptr[l + 1]; q++) {
      const int f = S.gn_level_fronts[q];
      const int r = 3 * S.fronts[f].ns;
      const int nchunk = std::max(1, (r + chunk_rows - 1) / chunk_rows);
      for (int c = 0; c < nchunk; c++) {
        WorkRec& wr = work[w++];
        memset(&wr, 0, sizeof wr);
        wr.F = S.fronts[f];
        wr.front = f;
        wr.chunk = c;
        for (int k = 0; k < std::min<int>(wr.F.nchild, kWorkChildren); k++) {
          const FrontDesc& G = S.fronts[S.children[wr.F.child_off + k]];
          WorkChild& wc = wr.ch[k];
          wc.U_off = G.U_off; wc.ns = G.ns; wc.na = G.na;
          wc.rel_off = G.rel_off; wc.inv_off = G.inv_off; wc.rows_off = G.rows_off;
        }
      }
    }
    if (w != D.h_work_ptr[l + 1]) return -1;
  }
  return n_work;
}
