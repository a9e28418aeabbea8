// Host side of the Gauss-Newton path (gn_host.h): errors, side stream, arenas, structure upload, the numeric pass, gn_run.
// Compiled with hipcc; contains no kernels.
#include "gn_host.h"
#include "init_device.h"

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstring>

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
int analyze_next(Symbolic& sym, const Switches& sw, bool have_prev, int prev_nV, const std::vector<int32_t>& pef, const std::vector<int32_t>& pet,
                 const GnSystem& N, const AnalyzeHooks* hooks) {
  int n_common = 0;
  if (have_prev && N.nV >= prev_nV && !pef.empty()) {
    const int lim = std::min(N.nE, (int)pef.size());
    while (n_common < lim && pef[n_common] == N.ef[n_common] && pet[n_common] == N.et[n_common]) n_common++;
  }
  const int old_nE = (int)pef.size();
  const bool grown = n_common > 0 && (n_common == old_nE || (N.n_hub_vertices > 0 && 2 * n_common >= old_nE));
  if (grown) {
    Symbolic old = std::move(sym);
    return analyze(N.nV, nullptr, N.nE, N.ef, N.et, sym, sw, &old, n_common == old_nE && N.nE >= old_nE ? -1 : n_common, N.hub_vertices, N.n_hub_vertices, hooks);
  }
  return analyze(N.nV, nullptr, N.nE, N.ef, N.et, sym, sw, nullptr, -1, N.hub_vertices, N.n_hub_vertices, hooks);
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
  int rc = analyze_next(ctx->sym, ctx->sw, have_prev, ctx->sym_nV, ctx->sym_ef, ctx->sym_et, {nV, nullptr, nullptr, nE, ef, et, hub_vertices, n_hub_vertices}, &hooks);
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

int gn_run(cgmr_ctx* ctx, const GnSystem& S, const GnEdges& Ed, int iters, double* chi2_out) {
  GnCall call(ctx, S);
  int rc = call.prepare(Ed.n_active, iters);
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
    for (o.chi_slot = it0; o.chi_slot < iters; o.chi_slot++) gn_pass(ctx, S.d_poses, Ei, o);
    o.chi_only = true;
    gn_pass(ctx, S.d_poses, Ed, o);
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
    gn_pass(ctx, S.d_poses, Ei, GnPassOpts());
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

void symbolic_info_out(const Symbolic& S, int nV, int64_t out[16], int32_t* perm_out) {
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

}  // namespace cgmr
