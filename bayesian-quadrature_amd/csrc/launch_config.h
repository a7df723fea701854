// launch_config.h -- the switches that decide which launches a call is made of (LaunchConfig), and
// a launch sequence captured into a hipGraph under them (CapturedSeq).  Depends on the HIP runtime
// API and on the status codes of include/bqhip.h only: tools/capture_check.hip compiles it alone.
#pragma once
#include <hip/hip_runtime.h>

#pragma GCC visibility push(default)
#include "../../include/bqhip.h"
#pragma GCC visibility pop

#include <cstdio>
#include <cstdlib>

// THE list of switches: X(member, environment name or nullptr, default), one entry per switch.
// LaunchConfig's members, the environment loop of a new context (LaunchConfig::from_env) and the
// comparison a captured graph is kept by all come from it; README.md names every environment
// switch with its test (tests/test_graph_replay.py holds the two lists together).  A field a
// setter writes belongs here too, or a captured graph outlives the setting it was captured under.
// clang-format off
#define BQ_LAUNCH_SWITCHES(X)                                                                       \
    X(lookahead, "BQ_LOOKAHEAD", 1)                                                                 \
    /* look-ahead only while the bulk update has at least this many rows (BQ_LA_MIN) */             \
    X(la_min, "BQ_LA_MIN", 3072)                                                                    \
    /* batches: every outer block as diagonal factor, ONE panel solve, update                       \
       (enqueue_potrf_dfirst; BQ_DIAG_FIRST=0: the recursive panels) */                             \
    X(diag_first, "BQ_DIAG_FIRST", 1)                                                               \
    /* the panel solve of an outer block in one launch (trsm_sweep_kernel; BQ_DF_SWEEP) */          \
    X(df_sweep, "BQ_DF_SWEEP", 1)                                                                   \
    /* a batch's diagonal factor by one workgroup per matrix (potrf_wg_kernel): -1 by batch size    \
       (potrf.hip, dfirst_wg), 0 / 1 forced (BQ_DF_WG) */                                           \
    X(df_wg, "BQ_DF_WG", -1)                                                                        \
    /* ... and, below that batch size, for the blocks with at least this many rows below them: the  \
       factors an update hides (BQ_DF_WG_ROWS; 0: never) */                                         \
    X(df_wg_rows, "BQ_DF_WG_ROWS", 1000)                                                            \
    /* the diagonal-first sweep forks before the panel solve: the next diagonal block's rows are    \
       solved, updated and factored beside the rest of the solve (BQ_DF_EARLY) */                   \
    X(df_early, "BQ_DF_EARLY", 1)                                                                   \
    /* single-vector sweeps as one launch each, hand-offs through memory (trsvflow.h;               \
       BQ_TRSV_FLOW=0: one launch per block column) */                                              \
    X(trsv_flow, "BQ_TRSV_FLOW", 1)                                                                 \
    /* bq_pair_esm as S factorisations + border rows (BQ_PAIR_BORDER=0: the S Ma full bordered      \
       systems) */                                                                                  \
    X(pair_border, "BQ_PAIR_BORDER", 1)                                                             \
    /* a one-vector solve's vector in / out and sentinel fill by kernels (BQ_SOLVE_KCOPY) */        \
    X(solve_kcopy, "BQ_SOLVE_KCOPY", 1)                                                             \
    /* LDS-staged 128x128 trailing update (BQ_GEMM_LDS) */                                          \
    X(gemm_lds, "BQ_GEMM_LDS", 1)                                                                   \
    /* one-launch sweeps carry their read-out (SlabOut; BQ_FOLD_READOUT) */                         \
    X(fold_readout, "BQ_FOLD_READOUT", 1)                                                           \
    /* a batched plan assembles only the first outer block's columns; the rest of the system is     \
       computed inside the first products that touch it (GramSeed; BQ_ASM_FUSE=0: the whole system  \
       is assembled first) */                                                                       \
    X(asm_fuse, "BQ_ASM_FUSE", 1)                                                                   \
    /* the one-launch steps' diagonal factor on eight waves where a step's workgroups have a CU     \
       each (BQ_POTF2_8W) */                                                                        \
    X(potf2_8w, "BQ_POTF2_8W", 1)                                                                   \
    /* the assembly's workgroup (0, 0) computes the leading block in the factor's registers         \
       (assemble_first_kernel; BQ_FIRST_REGS=0: stored, drained, reloaded) */                       \
    X(first_regs, "BQ_FIRST_REGS", 1)                                                               \
    /* ... and a slab step's 512-thread form while the step has at most this many workgroups per    \
       CU (launch_slab_step: no limit shipped; BQ_SLAB8_ROUNDS, 0: one) */                          \
    X(slab8_rounds, "BQ_SLAB8_ROUNDS", 1 << 20)                                                     \
    /* ... whose diagonal tiles are updated by waves 4-7, one k-block behind waves 0-3's solve      \
       (slab_step_kernel; BQ_DIAG_PIPE=0: solve, barrier, update on waves 0-3) */                   \
    X(diag_pipe, "BQ_DIAG_PIPE", 1)                                                                 \
    /* ... and whose tiles are stored write-through while the step's workgroups all run in one      \
       round: their write-back under workgroup 0's chain, not at the launch's end (slab_step_kernel, \
       WT; BQ_TILE_WT=0: plain stores) */                                                           \
    X(tile_wt, "BQ_TILE_WT", 1)                                                                     \
    /* eight-wave k-split forms of the 64-tile / job kernels (BQ_GEMM_KSPLIT) */                    \
    X(gemm_ksplit, "BQ_GEMM_KSPLIT", 1)                                                             \
    /* 64 / 128: force the LDS kernel's workgroup tile (BQ_GEMM_TILE; measurements) */              \
    X(gemm_tile, "BQ_GEMM_TILE", 0)                                                                 \
    /* replay plans, the pair's objective and vector sweeps from a captured hipGraph (BQ_GRAPH=0    \
       disables) */                                                                                 \
    X(use_graph, "BQ_GRAPH", 1)                                                                     \
    /* the outer block of the blocked factorisation (bq_set_block; 0: auto_nb chooses) */           \
    X(nb_override, nullptr, 0)
// clang-format on

struct LaunchConfig {
#define X(member, env, def) int member = def;
    BQ_LAUNCH_SWITCHES(X)
#undef X
    // the defaults with every environment switch that is set applied
    static LaunchConfig from_env()
    {
        LaunchConfig cfg;
        static const struct {
            const char *env;
            int LaunchConfig::*member;
        } switches[] = {
#define X(member, env, def) {env, &LaunchConfig::member},
            BQ_LAUNCH_SWITCHES(X)
#undef X
        };
        for (const auto &sw : switches)
            if (const char *e = sw.env ? std::getenv(sw.env) : nullptr)
                cfg.*sw.member = std::atoi(e);
        return cfg;
    }
    // exact and whole: no hash, no list to forget
    friend bool operator==(const LaunchConfig &a, const LaunchConfig &b)
    {
#define X(member, env, def) if (a.member != b.member) return false;
        BQ_LAUNCH_SWITCHES(X)
#undef X
        return true;
    }
    friend bool operator!=(const LaunchConfig &a, const LaunchConfig &b) { return !(a == b); }
};

// bq_ctx_stats [1..3], counted in CapturedSeq::run and nowhere else
struct CaptureStats {
    long captures = 0; // graphs captured and instantiated
    long replays = 0;  // graph launches
    long drops = 0;    // graphs dropped because the configuration had changed
};

// One launch sequence over fixed buffers -- a plan's pass, the pair's objective, a fit's vector
// sweeps -- captured into a hipGraph once and replayed: the only code of the library that captures,
// instantiates, launches or destroys a graph.  The rules, stated once:
//   eligible     a call replays only with cfg.use_graph, outside the launch profiler, on a stream
//                of the context's own and while the launch helpers enqueue on it (cur == stream).
//                Any other call is enqueued eagerly and changes nothing: a graph that is ready
//                stays ready (replay resumes after bq_profile_enable(0) without a new capture).
//   stale        a ready graph captured under another LaunchConfig than the context's is dropped
//                and the sequence captured again in the same call.  The comparison is of the whole
//                config: a setter call therefore costs every live sequence one recapture at its
//                next use, a fit's sweep slots included although no setter changes their launches
//                -- the price of having no per-user list of the fields that matter.
//   capture      relaxed mode on the context's stream; once begun it is always ended.
//   failure      of begin, enqueue, end or instantiate: what exists is destroyed, the HIP error
//                cleared, the sequence unavailable (eager calls) until drop().
//   per call     exactly one of {graph launch, enqueue() outside capture}.
// Ctx is bq_ctx (cfg, prof, own_stream, cur, stream, graphs, err); enqueue returns a BQ status.
struct CapturedSeq {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    enum State { NotTried, Ready, Unavailable } state = NotTried;
    LaunchConfig cfg; // what `graph` was captured under
    CapturedSeq() = default;
    CapturedSeq(const CapturedSeq &) = delete;
    CapturedSeq &operator=(const CapturedSeq &) = delete;
    ~CapturedSeq() { drop(); }
    // both handles go (the graph must not be in flight); the next eligible run captures again
    void drop()
    {
        if (exec)
            (void)hipGraphExecDestroy(exec);
        if (graph)
            (void)hipGraphDestroy(graph);
        exec = nullptr;
        graph = nullptr;
        state = NotTried;
    }
    template <class Ctx, class F>
    int run(Ctx *c, F &&enqueue)
    {
        if (!c->cfg.use_graph || c->prof || !c->own_stream || c->cur != c->stream)
            return enqueue();
        if (state == Ready && cfg != c->cfg) {
            drop();
            ++c->graphs.drops;
        }
        if (state == NotTried) {
            state = Unavailable;
            cfg = c->cfg;
            if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed) == hipSuccess) {
                const int st = enqueue();
                const hipError_t e = hipStreamEndCapture(c->stream, &graph);
                if (st == BQ_OK && e == hipSuccess && graph &&
                    hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                    state = Ready;
                    ++c->graphs.captures;
                }
            }
            if (state != Ready) {
                exec = nullptr; // (a failed instantiate hands nothing out)
                drop();
                state = Unavailable;
                (void)hipGetLastError(); // clear; this and later calls go out eagerly
            }
        }
        if (state != Ready)
            return enqueue();
        const hipError_t e = hipGraphLaunch(exec, c->stream);
        if (e != hipSuccess) {
            std::snprintf(c->err, sizeof c->err, "hipGraphLaunch failed: %s", hipGetErrorString(e));
            return BQ_ERR_HIP;
        }
        ++c->graphs.replays;
        return BQ_OK;
    }
};
