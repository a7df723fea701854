// Host-side check of CapturedSeq (csrc/launch_config.h): when a launch sequence is captured,
// replayed, dropped and recaptured, and what a failure leaves behind -- for a machine WITHOUT a
// device.  The six graph / capture calls (and hipGetLastError) are this program's own: they hand out
// and take back handles from a set of live ones, so a handle released twice or never is seen, and
// they can be told to fail.  Nothing here touches a device.  Host code only, under the sanitizers:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined tools/capture_check.hip \
//       -o build/capture_check && build/capture_check
#include "../bayesian-quadrature_amd/csrc/launch_config.h"

#include <set>

static std::set<void *> live;
static int bad = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);         \
            ++bad;                                                        \
        }                                                                 \
    } while (0)

// ---- the stubs -------------------------------------------------------------------------------
static bool capturing = false;
static int n_begin = 0, n_end = 0, n_inst = 0, n_launch = 0, n_destroy = 0, n_cleared = 0;
static bool fail_begin = false, fail_end = false, fail_inst = false, fail_launch = false;

template <class T>
static T handle()
{
    static char pool[256];
    static size_t next = 0;
    void *p = &pool[next++];
    live.insert(p);
    return static_cast<T>(p);
}
static hipError_t let_go(void *h)
{
    EXPECT(live.erase(h) == 1); // (0: released twice, or never handed out)
    ++n_destroy;
    return hipSuccess;
}
hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode mode)
{
    EXPECT(mode == hipStreamCaptureModeRelaxed && !capturing);
    ++n_begin;
    if (fail_begin)
        return hipErrorUnknown;
    capturing = true;
    return hipSuccess;
}
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t *g)
{
    EXPECT(capturing);
    capturing = false;
    ++n_end;
    if (fail_end)
        return hipErrorStreamCaptureInvalidated;
    *g = handle<hipGraph_t>();
    return hipSuccess;
}
hipError_t hipGraphInstantiate(hipGraphExec_t *x, hipGraph_t g, hipGraphNode_t *, char *, size_t)
{
    EXPECT(live.count(g) == 1);
    ++n_inst;
    if (fail_inst)
        return hipErrorOutOfMemory;
    *x = handle<hipGraphExec_t>();
    return hipSuccess;
}
hipError_t hipGraphLaunch(hipGraphExec_t x, hipStream_t)
{
    EXPECT(live.count(x) == 1 && !capturing);
    ++n_launch;
    return fail_launch ? hipErrorUnknown : hipSuccess;
}
hipError_t hipGraphExecDestroy(hipGraphExec_t x) { return let_go(x); }
hipError_t hipGraphDestroy(hipGraph_t g) { return let_go(g); }
hipError_t hipGetLastError(void)
{
    ++n_cleared;
    return hipSuccess;
}

// ---- what CapturedSeq::run reads of a context --------------------------------------------------
struct Ctx {
    LaunchConfig cfg;
    bool prof = false, own_stream = true;
    hipStream_t stream = reinterpret_cast<hipStream_t>(&live), cur = stream;
    CaptureStats graphs;
    char err[512] = {0};
};

// the sequence under test: counts its calls inside and outside a capture
static int n_in = 0, n_out = 0, enqueue_status = BQ_OK;
static int enqueue()
{
    ++(capturing ? n_in : n_out);
    return enqueue_status;
}

// every counter the checks look at, so that one comparison says "nothing else moved"
struct Counts {
    int in, out, begin, end, inst, launch, destroy;
    long captures, replays, drops;
    bool operator==(const Counts &o) const
    {
        return in == o.in && out == o.out && begin == o.begin && end == o.end && inst == o.inst &&
               launch == o.launch && destroy == o.destroy && captures == o.captures &&
               replays == o.replays && drops == o.drops;
    }
};
static Counts now(const Ctx &c)
{
    return {n_in, n_out, n_begin, n_end, n_inst, n_launch, n_destroy,
            c.graphs.captures, c.graphs.replays, c.graphs.drops};
}
// b = a + (the given steps)
static Counts plus(Counts a, int in, int out, int begin, int end, int inst, int launch, int destroy,
                   long captures, long replays, long drops)
{
    return {a.in + in, a.out + out, a.begin + begin, a.end + end, a.inst + inst, a.launch + launch,
            a.destroy + destroy, a.captures + captures, a.replays + replays, a.drops + drops};
}

int main()
{
    // 1. capture on the first run, launch only on the second; an unchanged setter value does
    //    neither, a changed member drops each handle once and captures again in the same call
    {
        Ctx c;
        CapturedSeq s;
        Counts t = now(c);
        EXPECT(s.run(&c, enqueue) == BQ_OK);
        EXPECT(now(c) == plus(t, 1, 0, 1, 1, 1, 1, 0, 1, 1, 0));
        EXPECT(s.state == CapturedSeq::Ready && live.size() == 2);
        t = now(c);
        EXPECT(s.run(&c, enqueue) == BQ_OK);
        EXPECT(now(c) == plus(t, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0));
        c.cfg.lookahead = 1; // (a setter called with the value in force)
        t = now(c);
        EXPECT(s.run(&c, enqueue) == BQ_OK);
        EXPECT(now(c) == plus(t, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0));
        // every member of the list counts, the ones launch_config_key left out included
#define X(member, env, def)                                                \
        {                                                                  \
            c.cfg.member += 1;                                             \
            t = now(c);                                                    \
            EXPECT(s.run(&c, enqueue) == BQ_OK);                           \
            EXPECT(now(c) == plus(t, 1, 0, 1, 1, 1, 1, 2, 1, 1, 1));       \
            EXPECT(s.state == CapturedSeq::Ready && live.size() == 2);     \
            EXPECT(s.cfg == c.cfg);                                        \
        }
        BQ_LAUNCH_SWITCHES(X)
#undef X
        // a launch that fails is reported, and the graph stays
        fail_launch = true;
        t = now(c);
        EXPECT(s.run(&c, enqueue) == BQ_ERR_HIP && c.err[0]);
        EXPECT(now(c) == plus(t, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0));
        EXPECT(s.state == CapturedSeq::Ready && live.size() == 2);
        fail_launch = false;
    } // 8. the destructor releases both handles
    EXPECT(live.empty());

    // 2. each failure: no live handle, unavailable, exactly one eager enqueue, the error cleared;
    //    once capture began it was ended.  drop() makes the sequence capturable again
    struct {
        const char *what;
        bool *flag;
        int begin, in, end, inst;
    } failures[] = {{"begin", &fail_begin, 1, 0, 0, 0},
                    {"end", &fail_end, 1, 1, 1, 0},
                    {"instantiate", &fail_inst, 1, 1, 1, 1},
                    {"enqueue", nullptr, 1, 1, 1, 0}};
    for (const auto &f : failures) {
        Ctx c;
        CapturedSeq s;
        if (f.flag)
            *f.flag = true;
        else
            enqueue_status = BQ_ERR_HIP;
        Counts t = now(c);
        const int cleared = n_cleared;
        const int st = s.run(&c, enqueue);
        EXPECT(st == (f.flag ? BQ_OK : BQ_ERR_HIP)); // (the eager call's own status)
        // (a graph that end or instantiate left behind is destroyed: 1 for instantiate and enqueue)
        const int destroyed = (f.inst || !f.flag) ? 1 : 0;
        EXPECT(now(c) == plus(t, f.in, 1, f.begin, f.end, f.inst, 0, destroyed, 0, 0, 0));
        EXPECT(s.state == CapturedSeq::Unavailable && live.empty() && !s.graph && !s.exec);
        EXPECT(n_cleared == cleared + 1 && !capturing);
        if (f.flag)
            *f.flag = false;
        else
            enqueue_status = BQ_OK;
        // it stays unavailable: eager, no new attempt ...
        t = now(c);
        EXPECT(s.run(&c, enqueue) == BQ_OK);
        EXPECT(now(c) == plus(t, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0));
        // ... until drop()
        s.drop();
        EXPECT(s.state == CapturedSeq::NotTried);
        t = now(c);
        EXPECT(s.run(&c, enqueue) == BQ_OK);
        EXPECT(now(c) == plus(t, 1, 0, 1, 1, 1, 1, 0, 1, 1, 0));
        EXPECT(s.state == CapturedSeq::Ready);
        if (bad)
            std::printf("(in the failure case \"%s\")\n", f.what);
    }
    EXPECT(live.empty());

    // 3. an ineligible context enqueues eagerly: a sequence not tried stays so, a ready graph stays
    //    ready (also one captured under another config) and is launched again afterwards
    for (int why = 0; why < 4; ++why) {
        Ctx c;
        CapturedSeq s;
        auto spoil = [&](bool on) {
            if (why == 0)
                c.cfg.use_graph = on ? 0 : 1;
            if (why == 1)
                c.prof = on;
            if (why == 2)
                c.own_stream = !on;
            if (why == 3)
                c.cur = on ? reinterpret_cast<hipStream_t>(&bad) : c.stream;
        };
        spoil(true);
        Counts t = now(c);
        EXPECT(s.run(&c, enqueue) == BQ_OK);
        EXPECT(now(c) == plus(t, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0));
        EXPECT(s.state == CapturedSeq::NotTried);
        spoil(false);
        EXPECT(s.run(&c, enqueue) == BQ_OK && s.state == CapturedSeq::Ready);
        spoil(true);
        if (why != 0)
            c.cfg.la_min += 1;
        t = now(c);
        EXPECT(s.run(&c, enqueue) == BQ_OK);
        EXPECT(now(c) == plus(t, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0));
        EXPECT(s.state == CapturedSeq::Ready && live.size() == 2);
        if (why != 0)
            c.cfg.la_min -= 1;
        spoil(false);
        t = now(c);
        EXPECT(s.run(&c, enqueue) == BQ_OK);
        EXPECT(now(c) == plus(t, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0));
    }
    EXPECT(live.empty());

    // 4. the environment reaches the member its entry names, and only that one
    {
        const LaunchConfig before = LaunchConfig::from_env();
        setenv("BQ_LA_MIN", "17", 1);
        LaunchConfig after = LaunchConfig::from_env();
        EXPECT(after.la_min == 17 && after != before);
        after.la_min = before.la_min;
        EXPECT(after == before);
    }
    std::printf(bad ? "%d check(s) FAILED\n" : "all checks passed\n", bad);
    return bad ? 1 : 0;
}
