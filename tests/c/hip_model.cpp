// hip_model.cpp -- see hip_model.h.  One mutex guards everything; the model is slow and simple on purpose.
#include "hip_model.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

namespace hipmodel {
namespace {

struct Alloc
{
    size_t bytes;
    int dev;   // -1: host-pinned
    uint64_t serial;
};
struct StreamRec
{
    int dev;
    bool null_stream;
    bool alive = true;
    uint64_t count = 0;             // operations queued
    std::vector<uint64_t> clock;    // by stream id
};
struct EventRec
{
    int dev;
    bool alive = true;
    std::vector<uint64_t> clock;    // frontier captured by the last hipEventRecord
};

std::mutex g_mu;
std::map<uintptr_t, Alloc> g_alloc;   // live allocations by address
std::vector<StreamRec> g_streams;     // ids 0 .. D-1 are the null streams of the devices
std::vector<std::unique_ptr<int>> g_stream_handles;   // a handle is the address of its id
std::vector<EventRec> g_events;
std::vector<std::unique_ptr<int>> g_event_handles;
std::vector<Op> g_log;
std::vector<uint64_t> g_host;         // what any host thread has waited for
std::map<std::thread::id, int> g_threads;
uint64_t g_serial = 0;
long g_fail_after = -1;
size_t g_violations = 0;
int g_devices = 0;

thread_local int t_device = 0;
thread_local std::vector<uint64_t> t_host;   // what THIS thread has waited for: ordered before what it queues next

void join(std::vector<uint64_t> &into, const std::vector<uint64_t> &from)
{
    if (into.size() < from.size()) into.resize(from.size(), 0);
    for (size_t i = 0; i < from.size(); i++) into[i] = std::max(into[i], from[i]);
}

void init_locked()
{
    if (g_devices) return;
    g_devices = 4;
    if (const char *e = getenv("HIP_MODEL_DEVICES"))
    {
        const int d = atoi(e);
        if (d >= 1 && d <= 8) g_devices = d;
    }
    for (int d = 0; d < g_devices; d++)
    {
        g_streams.push_back(StreamRec{d, true, true, 0, {}});
        g_stream_handles.emplace_back(new int(d));
    }
}

int thread_no_locked()
{
    auto it = g_threads.find(std::this_thread::get_id());
    if (it != g_threads.end()) return it->second;
    const int no = (int)g_threads.size();
    g_threads[std::this_thread::get_id()] = no;
    return no;
}

// id of a handle; -1 for one the model never made or has destroyed
int stream_id_locked(hipStream_t s, int device)
{
    if (!s) return device;
    for (size_t i = (size_t)g_devices; i < g_stream_handles.size(); i++)
        if ((void *)g_stream_handles[i].get() == (void *)s) return g_streams[i].alive ? (int)i : -1;
    return -1;
}
int event_id_locked(hipEvent_t e)
{
    for (size_t i = 0; i < g_event_handles.size(); i++)
        if ((void *)g_event_handles[i].get() == (void *)e) return g_events[i].alive ? (int)i : -1;
    return -1;
}

Op &new_op_locked(const char *kind)
{
    init_locked();
    g_log.emplace_back();
    Op &op    = g_log.back();
    op.kind   = kind;
    op.thread = thread_no_locked();
    op.device = t_device;
    return op;
}

void violate(Op &op, const std::string &what)
{
    op.violations.push_back(op.kind + ": " + what);
    g_violations++;
}

// host: the pointer may be ordinary host memory (one side of a copy); expect_dev: the device it must live on otherwise
void use_ptr(Op &op, const PtrArg &a, int expect_dev, bool host_ok)
{
    PtrUse u{a.name, a.p, a.bytes, -2, 0, 0};
    if (a.p)
    {
        const uintptr_t p = (uintptr_t)a.p;
        auto it           = g_alloc.upper_bound(p);
        if (it != g_alloc.begin() && (--it, p < it->first + it->second.bytes || (p == it->first && !it->second.bytes)))
        {
            u.alloc_dev = it->second.dev, u.serial = it->second.serial, u.offset = p - it->first;
            if (it->second.dev >= 0 && it->second.dev != expect_dev)
                violate(op, std::string(a.name) + " is memory of device " + std::to_string(it->second.dev) +
                                " used under device " + std::to_string(expect_dev));
            if (u.offset + a.bytes > it->second.bytes)
                violate(op, std::string(a.name) + " reaches " + std::to_string(u.offset + a.bytes) +
                                " bytes into an allocation of " + std::to_string(it->second.bytes) + " (past its end)");
        }
        else if (!host_ok)
            violate(op, std::string(a.name) + " is not inside a live allocation (unknown pointer)");
    }
    op.ptrs.push_back(u);
}

// puts the operation on its stream: position, clock, and the stream's device against the current device
void enqueue(Op &op, hipStream_t s)
{
    int id = stream_id_locked(s, t_device);
    if (id < 0)
    {
        violate(op, "stream is not a live stream of the model");
        id = t_device;
    }
    StreamRec &st = g_streams[(size_t)id];
    if (st.dev != t_device)
        violate(op, "stream " + stream_name(id) + " belongs to device " + std::to_string(st.dev) +
                        " but the current device is " + std::to_string(t_device));
    join(st.clock, t_host);
    if (st.clock.size() <= (size_t)id) st.clock.resize((size_t)id + 1, 0);
    st.clock[(size_t)id] = ++st.count;
    op.stream            = id;
    op.seq               = st.count;
    op.clock             = st.clock;
}

void host_waits(const std::vector<uint64_t> &clock)
{
    join(t_host, clock);
    join(g_host, clock);
}

bool device_ok(int d) { return d >= 0 && d < g_devices; }

hipError_t alloc(const char *kind, void **p, size_t bytes, int dev)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op = new_op_locked(kind);
    if (!p) return hipErrorInvalidValue;
    *p = nullptr;
    if (g_fail_after == 0)
    {
        g_fail_after = -1;
        op.kind += " (injected failure)";
        return hipErrorOutOfMemory;
    }
    if (g_fail_after > 0) g_fail_after--;
    const size_t rounded = (bytes + 255) / 256 * 256;
    void *mem            = aligned_alloc(256, rounded ? rounded : 256);
    if (!mem) return hipErrorOutOfMemory;
    memset(mem, 0, rounded ? rounded : 256);
    g_alloc[(uintptr_t)mem] = Alloc{bytes, dev, ++g_serial};
    op.ptrs.push_back(PtrUse{"p", mem, bytes, dev, g_serial, 0});
    *p = mem;
    return hipSuccess;
}

hipError_t release(const char *kind, void *p, bool pinned)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op = new_op_locked(kind);
    if (!p) return hipSuccess;
    auto it = g_alloc.find((uintptr_t)p);
    if (it == g_alloc.end() || (it->second.dev < 0) != pinned)
    {
        violate(op, "free of an unknown pointer");
        return hipErrorInvalidValue;
    }
    g_alloc.erase(it);
    free(p);
    return hipSuccess;
}

hipError_t copy(const char *kind, void *dst, const void *src, size_t bytes, hipMemcpyKind k, hipStream_t s, bool blocking)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op      = new_op_locked(kind);
    op.work     = true;
    op.blocking = blocking;
    use_ptr(op, ptr("dst", dst, bytes), t_device, k == hipMemcpyDeviceToHost || k == hipMemcpyDefault || k == hipMemcpyHostToHost);
    use_ptr(op, ptr("src", src, bytes), t_device, k == hipMemcpyHostToDevice || k == hipMemcpyDefault || k == hipMemcpyHostToHost);
    enqueue(op, s);
    if (op.violations.empty() && bytes) memmove(dst, src, bytes);
    if (blocking) host_waits(op.clock);
    return hipSuccess;
}

hipError_t fill(const char *kind, void *dst, int value, size_t bytes, hipStream_t s, bool blocking)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op      = new_op_locked(kind);
    op.work     = true;
    op.blocking = blocking;
    use_ptr(op, ptr("dst", dst, bytes), t_device, false);
    enqueue(op, s);
    if (op.violations.empty() && bytes) memset(dst, value, bytes);
    if (blocking) host_waits(op.clock);
    return hipSuccess;
}

}  // namespace

// ---- queries ---------------------------------------------------------------------------------------------------------
size_t log_size()
{
    std::lock_guard<std::mutex> lk(g_mu);
    return g_log.size();
}
Op log_op(size_t i)
{
    std::lock_guard<std::mutex> lk(g_mu);
    return g_log.at(i);
}
size_t violation_count()
{
    std::lock_guard<std::mutex> lk(g_mu);
    return g_violations;
}
std::vector<std::string> violations(size_t from, size_t to)
{
    std::lock_guard<std::mutex> lk(g_mu);
    std::vector<std::string> out;
    for (size_t i = from; i < to && i < g_log.size(); i++)
        for (const std::string &v : g_log[i].violations) out.push_back(v);
    return out;
}
std::string stream_name(int id)
{
    // no lock: called with and without it, on ids the caller got from the model
    if (id < 0) return "none";
    const StreamRec &s = g_streams[(size_t)id];
    return (s.null_stream ? std::string("null") : "s" + std::to_string(id)) + "@" + std::to_string(s.dev);
}
int stream_id(hipStream_t s, int device)
{
    std::lock_guard<std::mutex> lk(g_mu);
    init_locked();
    return stream_id_locked(s, device);
}
int stream_device(int id)
{
    std::lock_guard<std::mutex> lk(g_mu);
    return g_streams.at((size_t)id).dev;
}
uint64_t stream_position(int id)
{
    std::lock_guard<std::mutex> lk(g_mu);
    return g_streams.at((size_t)id).count;
}
bool is_null_stream(int id)
{
    std::lock_guard<std::mutex> lk(g_mu);
    return g_streams.at((size_t)id).null_stream;
}
int current_device() { return t_device; }
size_t live_allocations()
{
    std::lock_guard<std::mutex> lk(g_mu);
    return g_alloc.size();
}
size_t live_streams()
{
    std::lock_guard<std::mutex> lk(g_mu);
    size_t n = 0;
    for (const StreamRec &s : g_streams) n += s.alive && !s.null_stream;
    return n;
}
size_t live_events()
{
    std::lock_guard<std::mutex> lk(g_mu);
    size_t n = 0;
    for (const EventRec &e : g_events) n += e.alive;
    return n;
}
uint64_t allocations_made()
{
    std::lock_guard<std::mutex> lk(g_mu);
    return g_serial;
}

bool ordered_after_entry(size_t i, int S, uint64_t entry)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const Op &op = g_log.at(i);
    return (size_t)S < op.clock.size() && op.clock[(size_t)S] >= entry && (op.stream != S || op.seq > entry);
}
static bool before(const Op &op, const std::vector<uint64_t> &clock)
{
    return op.stream >= 0 && (size_t)op.stream < clock.size() && clock[(size_t)op.stream] >= op.seq;
}
bool joined(size_t i, int S)
{
    std::lock_guard<std::mutex> lk(g_mu);
    return before(g_log.at(i), g_streams.at((size_t)S).clock) || before(g_log.at(i), g_host);
}
bool joined_host(size_t i)
{
    std::lock_guard<std::mutex> lk(g_mu);
    return before(g_log.at(i), g_host);
}

hipError_t record_launch(const char *name, hipStream_t stream, const PtrArg *ptrs, size_t count)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op    = new_op_locked(name);
    op.work   = true;
    op.launch = true;
    for (size_t i = 0; i < count; i++) use_ptr(op, ptrs[i], t_device, false);
    enqueue(op, stream);
    return hipSuccess;
}

}  // namespace hipmodel

using namespace hipmodel;

extern "C" {

void hip_model_fail_alloc_after(long k)
{
    std::lock_guard<std::mutex> lk(g_mu);
    g_fail_after = k;
}

hipError_t hipGetDeviceCount(int *count)
{
    std::lock_guard<std::mutex> lk(g_mu);
    new_op_locked("hipGetDeviceCount");
    *count = g_devices;
    return hipSuccess;
}
hipError_t hipSetDevice(int device)
{
    std::lock_guard<std::mutex> lk(g_mu);
    new_op_locked("hipSetDevice");
    if (!device_ok(device)) return hipErrorInvalidDevice;
    t_device = device;
    return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int *value, hipDeviceAttribute_t attr, int device)
{
    std::lock_guard<std::mutex> lk(g_mu);
    new_op_locked("hipDeviceGetAttribute");
    if (!device_ok(device)) return hipErrorInvalidDevice;
    *value = attr == hipDeviceAttributeMultiprocessorCount ? 256 : 0;
    return hipSuccess;
}
hipError_t hipDeviceCanAccessPeer(int *can, int device, int peer)
{
    std::lock_guard<std::mutex> lk(g_mu);
    new_op_locked("hipDeviceCanAccessPeer");
    if (!device_ok(device) || !device_ok(peer)) return hipErrorInvalidDevice;
    *can = device != peer;
    return hipSuccess;
}
hipError_t hipDeviceEnablePeerAccess(int peer, unsigned int)
{
    std::lock_guard<std::mutex> lk(g_mu);
    new_op_locked("hipDeviceEnablePeerAccess");
    return device_ok(peer) && peer != t_device ? hipSuccess : hipErrorInvalidDevice;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory (model)" : "error (model)"; }

hipError_t hipMalloc(void **p, size_t bytes) { return alloc("hipMalloc", p, bytes, t_device); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return alloc("hipHostMalloc", p, bytes, -1); }
hipError_t hipFree(void *p) { return release("hipFree", p, false); }
hipError_t hipHostFree(void *p) { return release("hipHostFree", p, true); }

hipError_t hipPointerGetAttributes(hipPointerAttribute_t *a, const void *p)
{
    std::lock_guard<std::mutex> lk(g_mu);
    new_op_locked("hipPointerGetAttributes");
    auto it = g_alloc.upper_bound((uintptr_t)p);
    if (it == g_alloc.begin() || (--it, (uintptr_t)p >= it->first + std::max<size_t>(it->second.bytes, 1)))
        return hipErrorInvalidValue;
    memset(a, 0, sizeof(*a));
    a->type          = it->second.dev < 0 ? hipMemoryTypeHost : hipMemoryTypeDevice;
    a->device        = it->second.dev < 0 ? 0 : it->second.dev;
    a->devicePointer = (void *)p;
    a->hostPointer   = it->second.dev < 0 ? (void *)p : nullptr;
    return hipSuccess;
}

hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind k)
{
    return copy("hipMemcpy", dst, src, bytes, k, nullptr, true);
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind k, hipStream_t s)
{
    return copy("hipMemcpyAsync", dst, src, bytes, k, s, false);
}
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                            hipMemcpyKind k, hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op  = new_op_locked("hipMemcpy2DAsync");
    op.work = true;
    if (width > dpitch || width > spitch) violate(op, "width exceeds a pitch");
    const size_t dbytes = height ? (height - 1) * dpitch + width : 0, sbytes = height ? (height - 1) * spitch + width : 0;
    use_ptr(op, ptr("dst", dst, dbytes), t_device, k == hipMemcpyDeviceToHost || k == hipMemcpyDefault);
    use_ptr(op, ptr("src", src, sbytes), t_device, k == hipMemcpyHostToDevice || k == hipMemcpyDefault);
    enqueue(op, s);
    if (op.violations.empty())
        for (size_t r = 0; r < height; r++) memmove((char *)dst + r * dpitch, (const char *)src + r * spitch, width);
    return hipSuccess;
}
hipError_t hipMemcpyPeerAsync(void *dst, int dst_dev, const void *src, int src_dev, size_t bytes, hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op      = new_op_locked("hipMemcpyPeerAsync");
    op.work     = true;
    op.peer_dst = dst_dev, op.peer_src = src_dev;
    if (!device_ok(dst_dev) || !device_ok(src_dev)) violate(op, "names a device that does not exist");
    use_ptr(op, ptr("dst", dst, bytes), dst_dev, false);
    use_ptr(op, ptr("src", src, bytes), src_dev, false);
    enqueue(op, s);
    if (op.violations.empty() && bytes) memmove(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemset(void *dst, int value, size_t bytes) { return fill("hipMemset", dst, value, bytes, nullptr, true); }
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t s)
{
    return fill("hipMemsetAsync", dst, value, bytes, s, false);
}

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int flags)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op = new_op_locked("hipStreamCreateWithFlags");
    if (flags != hipStreamNonBlocking) violate(op, "a stream that is not hipStreamNonBlocking: the model orders no stream against the null stream");
    g_streams.push_back(StreamRec{t_device, false, true, 0, {}});
    g_stream_handles.emplace_back(new int((int)g_streams.size() - 1));
    *s = (hipStream_t)(void *)g_stream_handles.back().get();
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op       = new_op_locked("hipStreamDestroy");
    const int id = s ? stream_id_locked(s, 0) : -1;
    if (id < 0)
    {
        violate(op, "destroy of an unknown stream");
        return hipErrorInvalidValue;
    }
    g_streams[(size_t)id].alive = false;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op       = new_op_locked("hipStreamSynchronize");
    op.blocking  = true;
    const int id = stream_id_locked(s, t_device);
    if (id < 0)
    {
        violate(op, "synchronize of an unknown stream");
        return hipErrorInvalidValue;
    }
    op.stream = id;
    op.seq    = 0;
    host_waits(g_streams[(size_t)id].clock);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op      = new_op_locked("hipDeviceSynchronize");
    op.blocking = true;
    for (const StreamRec &s : g_streams)
        if (s.dev == t_device) host_waits(s.clock);
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op       = new_op_locked("hipStreamWaitEvent");
    const int id = stream_id_locked(s, t_device), ev = event_id_locked(e);
    if (id < 0 || ev < 0)
    {
        violate(op, "wait on an unknown stream or event");
        return hipErrorInvalidValue;
    }
    op.stream = id;
    join(g_streams[(size_t)id].clock, g_events[(size_t)ev].clock);
    return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned int)
{
    std::lock_guard<std::mutex> lk(g_mu);
    new_op_locked("hipEventCreateWithFlags");
    g_events.push_back(EventRec{t_device, true, {}});
    g_event_handles.emplace_back(new int((int)g_events.size() - 1));
    *e = (hipEvent_t)(void *)g_event_handles.back().get();
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op       = new_op_locked("hipEventDestroy");
    const int ev = event_id_locked(e);
    if (ev < 0)
    {
        violate(op, "destroy of an unknown event");
        return hipErrorInvalidValue;
    }
    g_events[(size_t)ev].alive = false;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op       = new_op_locked("hipEventRecord");
    const int id = stream_id_locked(s, t_device), ev = event_id_locked(e);
    if (id < 0 || ev < 0)
    {
        violate(op, "record with an unknown stream or event");
        return hipErrorInvalidValue;
    }
    if (g_streams[(size_t)id].dev != g_events[(size_t)ev].dev)
        violate(op, "event of device " + std::to_string(g_events[(size_t)ev].dev) + " recorded on stream " + stream_name(id));
    op.stream = id;
    join(g_streams[(size_t)id].clock, t_host);
    g_events[(size_t)ev].clock = g_streams[(size_t)id].clock;
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Op &op       = new_op_locked("hipEventSynchronize");
    op.blocking  = true;
    const int ev = event_id_locked(e);
    if (ev < 0)
    {
        violate(op, "synchronize of an unknown event");
        return hipErrorInvalidValue;
    }
    host_waits(g_events[(size_t)ev].clock);
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t)
{
    std::lock_guard<std::mutex> lk(g_mu);
    new_op_locked("hipEventElapsedTime");
    *ms = 0.0f;
    return hipSuccess;
}
}
