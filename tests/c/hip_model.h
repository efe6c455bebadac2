// hip_model.h -- a CPU model of the 28 HIP runtime calls the library's host half makes (tests/test_host_model.py).
// Plain C++17, built with g++ and linked in place of the runtime: allocations are zero-filled host memory with a
// device tag, copies and memsets move bytes at once, launches (tests/c/launch_model.cpp) are recorded and do nothing.
// What the model keeps is ORDER and PROVENANCE: every operation is logged with its thread, current device, stream and
// pointers, a vector clock per stream gives happens-before, and a pointer is checked against the allocation, the
// device and the stream it is used with.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <string>
#include <vector>

namespace hipmodel {

// One pointer of an operation.  bytes = 0: only the pointer itself is checked.
struct PtrArg
{
    const char *name;
    const void *p;
    size_t bytes;
};
inline PtrArg ptr(const char *name, const void *p, size_t bytes = 0) { return PtrArg{name, p, bytes}; }

struct PtrUse
{
    std::string name;
    const void *p;
    size_t bytes;
    int alloc_dev;      // device of the allocation, -1 host-pinned, -2 not inside a live allocation
    uint64_t serial;    // serial number of the allocation (0: none)
    size_t offset;      // of p inside the allocation
};

struct Op
{
    std::string kind;            // "hipMemcpyAsync", "launch_ct_rescale", ...
    int thread = 0;              // small number per host thread, in order of first appearance
    int device = 0;              // current device of the calling thread
    int stream = -1;             // id of the stream (index into the model's table), -1: not a stream operation
    uint64_t seq = 0;            // position on that stream
    bool work = false;           // a launch, copy or memset: something that reads or writes device memory
    bool launch = false;
    bool blocking = false;       // the call makes the host wait
    int peer_dst = -1, peer_src = -1;   // devices a peer copy names
    std::vector<PtrUse> ptrs;
    std::vector<uint64_t> clock; // by stream id: what is ordered before this operation (itself included)
    std::vector<std::string> violations;
};

// ---- the log ---------------------------------------------------------------------------------------------------------
size_t log_size();
Op log_op(size_t i);                     // a copy, taken under the model's mutex
size_t violation_count();                // over the whole log, including frees of unknown pointers
std::vector<std::string> violations(size_t from, size_t to);

std::string stream_name(int id);         // "s7@2", or "null@0" for the null stream of device 0
int stream_id(hipStream_t s, int device);   // device: whose null stream a NULL handle means
int stream_device(int id);
uint64_t stream_position(int id);        // operations queued on it so far
bool is_null_stream(int id);

int current_device();
size_t live_allocations();
size_t live_streams();
size_t live_events();
uint64_t allocations_made();             // successful allocations so far (device and pinned)

// ---- happens-before queries over a window [a, b) of the log -----------------------------------------------------------
// The caller's stream S had `entry` operations queued when the window began.
// ordered_after_entry: operation i comes after operation `entry` of S.
bool ordered_after_entry(size_t i, int S, uint64_t entry);
// joined: operation i is before S's frontier, or before what the host has waited for, as they stand now.
bool joined(size_t i, int S);
bool joined_host(size_t i);

// ---- recording (launch_model.cpp, and the driver's own wrong sequences) ---------------------------------------------
hipError_t record_launch(const char *name, hipStream_t stream, const PtrArg *ptrs, size_t count);
inline hipError_t record_launch(const char *name, hipStream_t stream, std::initializer_list<PtrArg> ptrs)
{
    return record_launch(name, stream, ptrs.begin(), ptrs.size());
}

}  // namespace hipmodel

extern "C" {
// Allocation number k + 1 from now (hipMalloc and hipHostMalloc alike) returns hipErrorOutOfMemory, once.  k < 0: off.
// The CPU allocator of a model; a GPU run has nothing like it.
void hip_model_fail_alloc_after(long k);
}
