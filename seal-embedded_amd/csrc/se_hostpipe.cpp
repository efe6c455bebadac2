// se_hostpipe.cpp -- see se_hostpipe.h.
#include "se_hostpipe.h"

#include <sched.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <deque>

#include "se_context.h"

namespace seamd {

// ---- memcpy pool ----------------------------------------------------------------------------
CopyPool::CopyPool(int nthreads) : nthreads_(std::max(1, nthreads))
{
    for (int i = 1; i < nthreads_; i++) workers_.emplace_back(&CopyPool::worker, this, i);
}

CopyPool::~CopyPool()
{
    {
        std::lock_guard<std::mutex> lk(mu_);
        stop_ = true;
        generation_++;
    }
    cv_job_.notify_all();
    for (auto &t : workers_) t.join();
}

static void copy_part(char *dst, const char *src, size_t bytes, int id, int nparts)
{
    // 4 KiB-aligned split so no two threads share a page of the destination
    size_t per = ((bytes + nparts - 1) / nparts + 4095) & ~size_t(4095);
    size_t lo  = std::min(bytes, per * id), hi = std::min(bytes, per * (id + 1));
    if (hi > lo) memcpy(dst + lo, src + lo, hi - lo);
}

void CopyPool::worker(int id)
{
    uint64_t seen = 0;
    for (;;)
    {
        char *dst;
        const char *src;
        size_t bytes;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_job_.wait(lk, [&] { return generation_ != seen; });
            seen = generation_;
            if (stop_) return;
            dst = dst_, src = src_, bytes = bytes_;
        }
        copy_part(dst, src, bytes, id, nthreads_);
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (--pending_ == 0) cv_done_.notify_one();
        }
    }
}

void CopyPool::copy(void *dst, const void *src, size_t bytes)
{
    if (nthreads_ == 1 || bytes < (size_t(1) << 20))
    {
        memcpy(dst, src, bytes);
        return;
    }
    {
        std::lock_guard<std::mutex> lk(mu_);
        dst_ = (char *)dst, src_ = (const char *)src, bytes_ = bytes;
        pending_ = nthreads_ - 1;
        generation_++;
    }
    cv_job_.notify_all();
    copy_part((char *)dst, (const char *)src, bytes, 0, nthreads_);
    std::unique_lock<std::mutex> lk(mu_);
    cv_done_.wait(lk, [&] { return pending_ == 0; });
}

static int default_copy_threads()
{
    if (const char *e = getenv("SE_AMD_HOST_THREADS"))
    {
        int v = atoi(e);
        if (v >= 1) return std::min(v, 64);
    }
    cpu_set_t set;
    int ncpu = 1;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) ncpu = CPU_COUNT(&set);
    return std::max(1, std::min(8, ncpu / 2));
}

// ---- pipeline -------------------------------------------------------------------------------
static bool is_pinned(const void *p)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess)
    {
        (void)hipGetLastError();  // unregistered host memory on older runtimes: not an error here
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// The slots and the ring wipe and free themselves (se_devmem.h) once both streams are drained.
HostPipe::~HostPipe()
{
    (void)hipSetDevice(device);
    if (compute) (void)hipStreamSynchronize(compute);
    if (copy) (void)hipStreamSynchronize(copy);
}

int HostPipe::init(int dev)
{
    device = dev;
    SEAMD_HIP(hipSetDevice(device));
    SEAMD_HIP(compute.create(hipStreamNonBlocking));
    SEAMD_HIP(copy.create(hipStreamNonBlocking));
    for (auto &s : slot)
    {
        SEAMD_HIP(s.computed.create(hipEventDisableTiming));
        SEAMD_HIP(s.copied.create(hipEventDisableTiming));
    }
    for (auto &r : ring) SEAMD_HIP(r.ev.create(hipEventDisableTiming));
    pool = std::make_unique<CopyPool>(default_copy_threads());
    return 0;
}

int HostPipe::ensure(Context &c, size_t chunk, size_t B, bool want_ntt, bool want_pte, bool staged)
{
    const size_t n = c.hp.n, ct_words = c.hp.nprimes * n;
    for (auto &s : slot)
    {
        if (s.values.size() < chunk * (n / 2) || s.seeds.size() < chunk * 64 || s.share_seeds.size() < chunk * 64 ||
            s.c0.size() < chunk * ct_words || s.c1.size() < chunk * ct_words)
        {
            // the wipes of the secret buffers run on the null stream, which does not order against the NON-BLOCKING
            // compute / copy streams: drain them first instead of relying on the callers having done so
            SEAMD_HIP(hipStreamSynchronize(compute));
            SEAMD_HIP(hipStreamSynchronize(copy));
            SEAMD_HIP(s.values.grow(chunk * (n / 2)));
            SEAMD_HIP(s.seeds.grow(chunk * 64));
            SEAMD_HIP(s.share_seeds.grow(chunk * 64));
            SEAMD_HIP(s.c0.grow(chunk * ct_words));
            SEAMD_HIP(s.c1.grow(chunk * ct_words));
        }
        if (want_ntt) SEAMD_HIP(s.ntt_pte.grow(chunk * ct_words));
        if (want_pte) SEAMD_HIP(s.pte.grow(chunk * n));
    }
    SEAMD_HIP(d_status.grow(B));
    SEAMD_HIP(h_status.grow((std::max<size_t>(B, 4096) + 4095) & ~size_t(4095)));
    if (staged)
    {
        // ring entries sized to the work: a single small ciphertext must not pin 256 MiB
        size_t want = std::min(kPieceMax, std::max(chunk * ct_words * 4, chunk * n * 8));
        want        = (want + 4095) & ~size_t(4095);
        for (auto &r : ring) SEAMD_HIP(r.buf.grow(want));
    }
    return 0;
}

namespace {
struct Piece
{
    const char *src;
    char *dst;
    size_t bytes;
    size_t chunk;
    bool first, last, direct;
};
struct InFlight
{
    int r;
    char *dst;
    size_t bytes;
};
}  // namespace

int HostPipe::run(Context &c, bool asym, const float *values, size_t B, const uint8_t *share_seeds,
                  const uint8_t *seeds, uint32_t *c0, uint32_t *c1, uint32_t *ntt_pte, int64_t *pte,
                  uint8_t *status)
{
    const size_t n = c.hp.n, np = c.hp.nprimes;
    const size_t ct_bytes = np * n * 4;
    SEAMD_HIP(hipSetDevice(device));

    // chunk: enough ciphertexts to fill the chip's chain kernels (16384 = 256 CUs x 64 lanes) but no
    // more than 4 GiB per output slab; chunks equalised so there is no tiny tail
    size_t chunk_max = chunk_override
                           ? chunk_override
                           : std::min<size_t>(16384, std::max<size_t>(256, (size_t(4) << 30) / (2 * ct_bytes)));
    const size_t nchunks = (B + chunk_max - 1) / chunk_max;
    size_t chunk         = (B + nchunks - 1) / nchunks;
    if (!chunk_override) chunk = std::min(B, (chunk + 63) & ~size_t(63));
    const size_t nch = (B + chunk - 1) / chunk;

    // c1 == nullptr (symmetric only): seed-compressed form, `a` stays in the device slot
    const bool pin0 = is_pinned(c0), pin1 = !c1 || is_pinned(c1);
    const bool pinn = ntt_pte && is_pinned(ntt_pte), pinp = pte && is_pinned(pte);
    const bool staged = !pin0 || !pin1 || (ntt_pte && !pinn) || (pte && !pinp);
    int rc = ensure(c, chunk, B, ntt_pte != nullptr, pte != nullptr, staged);
    if (rc) return rc;

    auto chunk_count = [&](size_t k) { return std::min(chunk, B - k * chunk); };

    auto launch_chunk = [&](size_t k) -> int {
        Slot &s          = slot[k % kSlots];
        const size_t lo  = k * chunk, cnt = chunk_count(k);
        // inputs go through the runtime's pageable H2D path (staging them through own pinned buffers
        // with the memcpy pool measured 9 % slower end to end).  They are issued first: they only
        // depend on the previous use of this slot's input buffers (same
        // stream); the wait for the slot's outputs to be copied out comes after, so the (host
        // blocking) pageable H2D never waits on ring pieces this thread has yet to drain
        SEAMD_HIP(hipMemcpyAsync(s.values, values + lo * (n / 2), cnt * (n / 2) * sizeof(float),
                                 hipMemcpyHostToDevice, compute));
        SEAMD_HIP(hipMemcpyAsync(s.seeds, seeds + lo * 64, cnt * 64, hipMemcpyHostToDevice, compute));
        if (!asym)
            SEAMD_HIP(hipMemcpyAsync(s.share_seeds, share_seeds + lo * 64, cnt * 64,
                                     hipMemcpyHostToDevice, compute));
        if (k >= kSlots) SEAMD_HIP(hipStreamWaitEvent(compute, s.copied, 0));
        uint8_t *st = d_status + lo;
        uint32_t *s_ntt = ntt_pte ? s.ntt_pte.get() : nullptr;
        int64_t *s_pte  = pte ? s.pte.get() : nullptr;
        int r;
        if (asym)
            r = c.encrypt_asym(s.values, cnt, s.seeds, s.c0, s.c1, s_ntt, s_pte, st, compute);
        else
            r = c.encrypt_sym(s.values, cnt, s.share_seeds, s.seeds, s.c0, s.c1, s_ntt, s_pte, st, compute);
        if (r) return r;
        SEAMD_HIP(hipEventRecord(s.computed, compute));
        return 0;
    };

    // the D2H schedule: per chunk c0, c1, (ntt_pte), (pte); staged outputs in ring-sized pieces
    std::vector<Piece> pieces;
    size_t ring_bytes = kPieceMax;   // pieces staged through the ring fit every entry
    for (auto &r : ring) ring_bytes = std::min(ring_bytes, r.buf.size());
    for (size_t k = 0; k < nch; k++)
    {
        Slot &s         = slot[k % kSlots];
        const size_t lo = k * chunk, cnt = chunk_count(k);
        struct Out
        {
            const void *src;
            void *dst;
            size_t bytes;
            bool direct;
        } outs[4] = {
            {s.c0, (char *)c0 + lo * ct_bytes, cnt * ct_bytes, pin0},
            {s.c1, c1 ? (char *)c1 + lo * ct_bytes : nullptr, c1 ? cnt * ct_bytes : 0, pin1},
            {s.ntt_pte, ntt_pte ? (char *)ntt_pte + lo * ct_bytes : nullptr, ntt_pte ? cnt * ct_bytes : 0, pinn},
            {s.pte, pte ? (char *)pte + lo * n * 8 : nullptr, pte ? cnt * n * 8 : 0, pinp},
        };
        const size_t first_idx = pieces.size();
        for (auto &o : outs)
        {
            if (!o.bytes) continue;
            const size_t step = o.direct ? o.bytes : ring_bytes;
            for (size_t off = 0; off < o.bytes; off += step)
                pieces.push_back({(const char *)o.src + off, (char *)o.dst + off,
                                  std::min(step, o.bytes - off), k, false, false, o.direct});
        }
        pieces[first_idx].first = true;
        pieces.back().last      = true;
    }

    std::deque<InFlight> inflight;
    int failure    = 0;
    auto drain_one = [&]() -> int {
        InFlight f = inflight.front();
        inflight.pop_front();
        SEAMD_HIP(hipEventSynchronize(ring[f.r].ev));
        pool->copy(f.dst, ring[f.r].buf, f.bytes);
        return 0;
    };

    for (size_t k = 0; k < std::min<size_t>(kSlots, nch); k++)
        if ((rc = launch_chunk(k))) return rc;

    size_t ring_next = 0;
    for (const Piece &p : pieces)
    {
        Slot &s = slot[p.chunk % kSlots];
        if (p.first) SEAMD_HIP(hipStreamWaitEvent(copy, s.computed, 0));
        if (p.direct)
            SEAMD_HIP(hipMemcpyAsync(p.dst, p.src, p.bytes, hipMemcpyDeviceToHost, copy));
        else
        {
            while (inflight.size() == (size_t)kRing)
                if ((rc = drain_one())) { failure = rc; break; }
            if (failure) break;
            const int r = int(ring_next++ % kRing);
            SEAMD_HIP(hipMemcpyAsync(ring[r].buf, p.src, p.bytes, hipMemcpyDeviceToHost, copy));
            SEAMD_HIP(hipEventRecord(ring[r].ev, copy));
            inflight.push_back({r, p.dst, p.bytes});
        }
        if (p.last)
        {
            SEAMD_HIP(hipEventRecord(s.copied, copy));
            if (p.chunk + kSlots < nch && (rc = launch_chunk(p.chunk + kSlots))) { failure = rc; break; }
        }
    }
    // the status bytes ride the copy stream behind the last piece (every chunk has been launched by now and the
    // compute stream is in order, so the last chunk's `computed` event covers them all): no synchronous copy of
    // their own after the drain -- 15-20 us of a single call
    if (!failure)
    {
        hipError_t es = hipStreamWaitEvent(copy, slot[(nch - 1) % kSlots].computed, 0);
        if (es == hipSuccess) es = hipMemcpyAsync(h_status, d_status, B, hipMemcpyDeviceToHost, copy);
        if (es != hipSuccess) failure = hip_fail(es, "status download");
    }
    while (!failure && !inflight.empty()) failure = drain_one();
    // always quiesce both streams before returning (also on the error path: the slots are reused)
    hipError_t e1 = hipStreamSynchronize(copy), e2 = hipStreamSynchronize(compute);
    if (failure) return failure;
    if (e1 != hipSuccess) return hip_fail(e1, "hipStreamSynchronize(copy)");
    if (e2 != hipSuccess) return hip_fail(e2, "hipStreamSynchronize(compute)");

    int failed = 0;
    for (size_t i = 0; i < B; i++) failed += h_status[i] ? 0 : 1;
    if (status) memcpy(status, h_status, B);
    return failed;
}

}  // namespace seamd
