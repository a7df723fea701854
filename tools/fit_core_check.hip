// Host-side soundness of a fit's buffers (csrc/host.h: FitCore::alloc's failure path, fit_adopt, the
// drop() of a fit's three captured sweeps, fit_grow of the on-demand workspaces), for a machine
// WITHOUT a device: there every hipMalloc of the real runtime fails, which is the all-or-nothing path.  The release calls (hipFree, hipHostFree,
// hipGraphExecDestroy, hipGraphDestroy) are this program's own: they take a handle out of a set of
// live ones, so a handle freed twice or never is seen.  Host code only, under the sanitizers:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined tools/fit_core_check.hip \
//       -o build/fit_core_check && build/fit_core_check
#include "../bayesian-quadrature_amd/csrc/host.h"

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

static hipError_t let_go(void *h)
{
    EXPECT(live.erase(h) == 1); // (0: freed twice, or never handed out)
    return hipSuccess;
}
hipError_t hipFree(void *p) { return let_go(p); }
hipError_t hipHostFree(void *p) { return let_go(p); }
hipError_t hipGraphExecDestroy(hipGraphExec_t g) { return let_go(g); }
hipError_t hipGraphDestroy(hipGraph_t g) { return let_go(g); }

// a handle that is nothing but its value (never dereferenced: the release calls above are ours)
template <class T = void *>
static T handle()
{
    static char pool[256];
    static size_t next = 0;
    void *p = &pool[next++];
    live.insert(p);
    return static_cast<T>(p);
}
static void hold(DevBuf &b, size_t bytes)
{
    b.p = handle();
    b.bytes = bytes;
}

namespace bqh {
SweepRoute sweep_route(const bq_ctx *, int ntot, int ncols, int batch, size_t)
{
    SweepRoute r{};
    r.kind = SweepRoute::Slab;
    r.ntot = ntot, r.ncols = ncols, r.batch = batch;
    r.ws_doubles = (size_t)2 * 64 * ntot;
    return r;
}
} // namespace bqh

static bool empty(const FitCore &k)
{
    for (const DevBuf *b : {&k.A, &k.pts, &k.y, &k.dinv, &k.panel, &k.dw, &k.alpha})
        if (b->p || b->bytes || b->guard)
            return false;
    return k.npad == 0 && k.ldl == 0 && k.L.n == 0 && k.L.npad == 0 && k.L.ntot == 0;
}

int main()
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        std::printf("a device is present: hipMalloc would succeed, nothing to check here\n");
        return 0;
    }
    (void)hipGetLastError();
    bq_ctx c;

    // 1. a failed alloc leaves every pointer null and every size zero, and says so in the
    //    caller's words
    {
        FitCore k;
        const int st = k.alloc(&c, 2, 100, "check: the layout of %d points", 100);
        EXPECT(st == BQ_ERR_NOMEM || st == BQ_ERR_HIP);
        EXPECT(empty(k));
        EXPECT(std::strncmp(c.err, "check: the layout of 100 points: ", 33) == 0);
        std::printf("alloc without a device: status %d, \"%s\"\n", st, c.err);
        // ... also when it fails on a core that holds buffers (alloc releases what it replaces)
        for (DevBuf *b : {&k.A, &k.pts, &k.y, &k.dinv, &k.panel, &k.dw, &k.alpha})
            hold(*b, 64);
        EXPECT(k.alloc(&c, 2, 100, "again") != BQ_OK);
        EXPECT(empty(k) && live.empty());
    }

    // 2. adopting a core, then destroying the fit and the old core: every handle is let go once
    {
        bq_fit *f = new bq_fit();
        FitCore next;
        f->npad = 128, f->ldl = 192, f->L = bqh::make_layout(100, 0, true);
        next.npad = 192, next.ldl = 256, next.L = bqh::make_layout(140, 0, true);
        for (DevBuf *b : {&f->A, &f->pts, &f->y, &f->dinv, &f->panel, &f->dw, &f->alpha})
            hold(*b, 128);
        for (DevBuf *b : {&next.A, &next.pts, &next.y, &next.dinv, &next.panel, &next.dw, &next.alpha})
            hold(*b, 192);
        for (DevBuf *b : {&f->gp, &f->misc, &f->wide, &f->vec, &f->wV, &f->wV2, &f->wx, &f->wout,
                          &f->wz, &f->gY, &f->gX, &f->gpart, &f->hB, &f->loo})
            hold(*b, 128);
        f->hvec = handle<double *>(), f->hio = handle<double *>(), f->hfit = handle<double *>();
        for (int i = 0; i < 3; ++i) {
            f->vseq[i].graph = handle<hipGraph_t>();
            f->vseq[i].exec = handle<hipGraphExec_t>();
            f->vseq[i].state = CapturedSeq::Unavailable;
        }
        f->have = bq_fit::FACTOR_CHANGED;
        const size_t before = live.size();
        bqh::fit_adopt(f, next);
        // the ten workspaces sized by the padding, hvec and the six graph handles are gone ...
        EXPECT(live.size() == before - 10 - 1 - 6);
        EXPECT(!f->hvec && f->hio && f->hfit && f->gp.p && f->misc.p && f->wx.p && f->wout.p);
        for (int i = 0; i < 3; ++i)
            EXPECT(!f->vseq[i].graph && !f->vseq[i].exec && f->vseq[i].state == CapturedSeq::NotTried);
        // ... and the fit holds the new core, the caller the old one
        EXPECT(f->npad == 192 && f->ldl == 256 && f->L.n == 140 && f->A.bytes == 192);
        EXPECT(next.npad == 128 && next.ldl == 192 && next.L.n == 100 && next.alpha.bytes == 128);
        EXPECT(f->have == bq_fit::FACTOR_CHANGED); // (the caller drops the derived state)
        f->drop(bq_fit::TARGETS_CHANGED);
        EXPECT(f->have == (bq_fit::DW | bq_fit::WIDE));
        // ~bq_fit lets the graph handles of a live fit go as well, once each
        for (int i = 0; i < 3; ++i) {
            f->vseq[i].graph = handle<hipGraph_t>();
            f->vseq[i].exec = handle<hipGraphExec_t>();
            f->vseq[i].state = CapturedSeq::Ready;
        }
        delete f;
        EXPECT(live.size() == 7); // the old core, until it goes out of scope
    }
    EXPECT(live.empty());

    // 3. fit_grow, the one way an on-demand workspace of a fit grows: a failed allocation is a
    //    status, the caller's words and the byte count at the front of the message, and an empty
    //    buffer -- also where it replaces a smaller one, which is let go once
    {
        DevBuf b;
        const int st = bqh::fit_grow(&c, b, 4096, "check workspace");
        EXPECT(st == BQ_ERR_NOMEM || st == BQ_ERR_HIP);
        EXPECT(std::strncmp(c.err, "check workspace (4096 bytes): ", 30) == 0);
        EXPECT(!b.p && b.bytes == 0);
        std::printf("fit_grow without a device: status %d, \"%s\"\n", st, c.err);
        hold(b, 64);
        EXPECT(bqh::fit_grow(&c, b, 4096, "again") != BQ_OK);
        EXPECT(!b.p && b.bytes == 0 && live.empty());
        // a buffer that is large enough comes back untouched: no allocation was tried (here it
        // would have failed and left the buffer empty), no message written
        hold(b, 4096);
        void *const p = b.p;
        c.err[0] = 0;
        EXPECT(bqh::fit_grow(&c, b, 4096, "enough") == BQ_OK);
        EXPECT(bqh::fit_grow(&c, b, 100, "enough") == BQ_OK);
        EXPECT(b.p == p && b.bytes == 4096 && live.size() == 1 && c.err[0] == 0);
    }
    EXPECT(live.empty());
    std::printf(bad ? "%d check(s) FAILED\n" : "all checks passed\n", bad);
    return bad ? 1 : 0;
}
