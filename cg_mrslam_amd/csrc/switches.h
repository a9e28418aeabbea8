// Every environment switch of libcgmr.so: one table, one reader ("Environment switches"; tools/README.md lists
// the same table for the reader of a terminal).
//
// Scopes.  context: cgmr_ctx_create reads the switch into ctx->sw, and everything that works for that context -- its
// analyses, uploads, launches, matcher calls, robot graphs -- takes it from there; the entry points that analyse without a
// context (cgmr_gn_symbolic_info*, cgmr_debug_*, tests/host/symbolic_sweep.cpp) read the same switches when they are called.
// process: the switch configures an object the whole process shares (the helper pool, the RCCL library) and is read once,
// when that object is first needed (process_switches()).
//
// Kinds (how the variable's text becomes the value):
//   flag    set: whether atoi() reads its text as non-zero.  With default true the switch is on unless set to 0; with default
//           false it is opt-in
//   set     true if the variable is set at all, whatever its text (the traces)
//   num     atoi() of the variable, the default when it is not set
//   chunk   num, an explicit value held to [16, kChunkRows]
//   min0, min1   num, an explicit value raised to 0 / 1
//   text    the variable's text as it is, null when it is not set
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "gn_symbolic.h"

namespace cgmr {

// X(variable, field, kind, default, scope, effect)
#define CGMR_SWITCH_TABLE(X)                                                                                                        \
  /* launch shape of the solver */                                                                                                  \
  X("CGMR_FWD_MERGE", fwd_merge, flag, true, context, "a level's factorisation and update tiles in one launch where it is certainly resident; 0: two launches per level") \
  X("CGMR_FWD_MERGE_ANY", fwd_merge_any, flag, true, context, "merged level launches also where residency is not certain, until the context's first time-out; 0: never") \
  X("CGMR_BWD_CHAIN", bwd_chain, num, -1, context, "at most n workgroups in the chained backward solve; 0: one launch per level; -1: what is certainly resident") \
  X("CGMR_BWD_CHAIN_WGS", bwd_chain_wgs, num, 0, context, "2 / 4: that instance of the chained backward solve (workgroups per CU); else chosen by tree size") \
  X("CGMR_BWD_SPIN_LIMIT", bwd_spin_limit, min1, 1 << 22, context, "polls a bounded device-side wait may take (chained backward solve, merged levels) before it times out") \
  X("CGMR_TOP_BLOCK", top_block, flag, true, context, "the last fronts of the root's chain in one launch (k_top_block); 0: fronts like any other") \
  X("CGMR_CLEAR_IN_TOP", clear_in_top, flag, true, context, "the top-block launch clears the panels for the next pass; 0: a memset per pass") \
  X("CGMR_CHUNK", mid_chunk, chunk, kMidChunkRows, context, "border rows per work item above the leaves") \
  X("CGMR_LEAF_CHUNK", leaf_chunk, chunk, kLeafChunkRows, context, "border rows per work item on a level of leaves") \
  X("CGMR_TOP_CHUNK", top_chunk, chunk, kTopChunkRows, context, "border rows per work item on a level of at most CGMR_TOP_CHUNK_FRONTS fronts") \
  X("CGMR_TOP_CHUNK_FRONTS", top_chunk_fronts, num, kTopChunkFronts, context, "fronts a level may have to take CGMR_TOP_CHUNK") \
  X("CGMR_GRAPH", graph, flag, false, context, "capture one Gauss-Newton iteration into a hipGraph and replay it")                 \
  /* analysis */                                                                                                                    \
  X("CGMR_AMALGAMATE", amalgamate, flag, true, context, "merge a front into its parent where that is free; 0: one front per panel")  \
  X("CGMR_ND_REUSE_START", nd_reuse_start, flag, true, context, "a dissection node starts its sweep where the parent's ended; 0: its own far-vertex sweep") \
  X("CGMR_ND_ROOT_STARTS", nd_root_starts, num, 4, context, "structuring sweeps the root runs side by side (at most 16); 0 / 1: the double sweep") \
  X("CGMR_ND_INHERIT", nd_inherit, flag, true, context, "a dissection node takes the sweep its caller already holds (near half, first component); 0: it sweeps anew") \
  X("CGMR_ND_MIN_COVER", nd_min_cover, flag, true, context, "separator = minimum vertex cover between two levels; 0: the whole level") \
  X("CGMR_ND_PAR_DEPTH", nd_par_depth, num, -1, context, "dissection levels that fork a helper thread; -1: by the number of host threads") \
  X("CGMR_HUB_DEGREE", hub_degree, num, 32, context, "vertices of more neighbours are eliminated last (hubs); 0: no hubs, named ones included") \
  X("CGMR_SYM_EXTEND", sym_extend, flag, true, context, "a grown graph extends the cached ordering; 0: every analysis from scratch")  \
  X("CGMR_SYM_EXTEND_CHECK", sym_extend_check, flag, true, context, "an extension checks that new edges keep subtrees independent; 0: unchecked (a known-wrong structure)") \
  X("CGMR_SYM_EXTEND_SLACK", sym_extend_slack, num, 2, context, "panels an extended tree may be taller than the last from-scratch one; negative: no bound") \
  X("CGMR_ADJ_SLICES", adj_slices, flag, true, context, "adjacency built from per-thread slices of the edge list; 0: per-thread vertex ranges") \
  /* matcher and condensed graphs */                                                                                                \
  X("CGMR_MATCH_EDT", match_edt, flag, true, context, "rasterise by a distance transform where the kernel table allows it; 0: stamp the kernel per point") \
  X("CGMR_MATCH_SPLIT", match_split, min1, 16, context, "workgroups that may share one pair's search angles")                       \
  X("CGMR_MATCH_PRUNE", match_prune, flag, true, context, "drop candidates that cannot win when the bin count is not asked for; 0: score them all") \
  X("CGMR_MATCH_LEAN", match_lean, flag, true, context, "lean kernel instances for the usual batch shape, the general one behind them; 0: the general one only") \
  X("CGMR_MATCH_NOREDO", match_noredo, flag, false, context, "profiling only: pairs the lean instance hands back are not searched (their results are wrong)") \
  X("CGMR_HIER_HOST", hier_host, flag, false, context, "hierarchical search level by level from the host; default: the levels chained on the device") \
  X("CGMR_GUESS_CACHED", guess_cached, flag, true, context, "condensed graphs: initial guess by the cached spanning-tree walk; 0: the general edge-list walk") \
  /* traces (stderr) */                                                                                                             \
  X("CGMR_TRACE_LAUNCHES", trace_launches, set, false, context, "name every solver launch and synchronise after it")                \
  X("CGMR_GN_TRACE", gn_trace, set, false, context, "where a solve's wall time goes, summed, printed when the context is destroyed") \
  X("CGMR_SYM_TRACE", sym_trace, set, false, context, "the analysis' phases, one line each")                                        \
  X("CGMR_COND_TRACE", cond_trace, set, false, context, "the condensed-graph batch's phases")                                       \
  X("CGMR_MATCH_TRACE", match_trace, set, false, context, "the generic searches' stages, one line each")                            \
  /* host pool and RCCL: objects of the process */                                                                                  \
  X("CGMR_HOST_THREADS", host_threads, num, 0, process, "threads of an analysis, caller included (at most 16); 0: by CPU count and cgroup quota") \
  X("CGMR_HOST_PIN", host_pin, num, 1, process, "1: a helper per core around the creating CPU's cache group; 2: anywhere in that group; 0: not pinned") \
  X("CGMR_HOST_PIN_CALLER", host_pin_caller, flag, false, process, "hold the calling thread on the pool's home core while it analyses") \
  X("CGMR_HOST_MOVE", host_move, flag, false, process, "move the pool to another cache group when its cores are kept busy by others") \
  X("CGMR_HOST_STEAL", host_steal, flag, true, process, "a waiting caller runs its own queued jobs; 0: it only waits")                 \
  X("CGMR_HOST_SPIN_US", host_spin_us, min0, 200, process, "microseconds an idle helper spins before it sleeps")                    \
  X("CGMR_RCCL_LIB", rccl_lib, text, nullptr, process, "path of the RCCL library to load when the default names are not found")

namespace switch_kind {
typedef bool flag; typedef bool set;
typedef int num; typedef int chunk; typedef int min0; typedef int min1;
typedef const char* text;
}  // namespace switch_kind

struct Switches {
#define X(var, field, kind, def, scope, effect) switch_kind::kind field = def;
  CGMR_SWITCH_TABLE(X)
#undef X
};

namespace switch_parse {   // e: the variable's text, never null here
inline bool flag(const char* e) { return atoi(e) != 0; }
inline bool set(const char*) { return true; }
inline int num(const char* e) { return atoi(e); }
inline int chunk(const char* e) { return std::min(kChunkRows, std::max(16, atoi(e))); }
inline int min0(const char* e) { return std::max(0, atoi(e)); }
inline int min1(const char* e) { return std::max(1, atoi(e)); }
inline const char* text(const char* e) { return e; }
}  // namespace switch_parse

// The one place that reads CGMR_* variables: every switch of the table from the environment as it is now.
inline Switches read_switches() {
  Switches s;
#define X(var, field, kind, def, scope, effect) if (const char* e = getenv(var)) s.field = switch_parse::kind(e);
  CGMR_SWITCH_TABLE(X)
#undef X
  return s;
}

// The process-scoped switches (the others are not to be taken from here), read when first asked for.
inline const Switches& process_switches() {
  static const Switches s = read_switches();
  return s;
}

// "name<TAB>scope<TAB>value<TAB>effect\n" per switch into buf (cap bytes, always terminated when cap > 0); returns the bytes
// the whole listing needs, terminator included.  Context-scoped values from `ctx_sw`, process-scoped ones from `proc_sw`.
inline int list_switches(const Switches& ctx_sw, const Switches& proc_sw, char* buf, int cap) {
  struct Put {
    static int value(char* b, size_t n, bool v) { return snprintf(b, n, "%d", v ? 1 : 0); }
    static int value(char* b, size_t n, int v) { return snprintf(b, n, "%d", v); }
    static int value(char* b, size_t n, const char* v) { return snprintf(b, n, "%s", v ? v : ""); }
  };
  const Switches &context = ctx_sw, &process = proc_sw;
  size_t need = 0;
  auto room = [&](char*& at) { at = need < (size_t)std::max(cap, 0) ? buf + need : nullptr; return at ? (size_t)cap - need : 0; };
  char* at;
  size_t n;
#define X(var, field, kind, def, scope, effect)                         \
  n = room(at); need += snprintf(at, n, "%s\t%s\t", var, #scope);       \
  n = room(at); need += Put::value(at, n, scope.field);                 \
  n = room(at); need += snprintf(at, n, "\t%s\n", effect);
  CGMR_SWITCH_TABLE(X)
#undef X
  return (int)need + 1;
}

}  // namespace cgmr
