// What the HIP sources (device.hip, reach.hip, diff.hip) share on the host side of a launch: the
// error macro, the CU count, the resident grid and the owner of a call's scratch block. HIP only:
// no host .cpp file includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <string>

namespace pg {

// inside a function that returns int and has a `std::string* err`
#define HIPCHK(expr)                                                         \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) {                                              \
            if (err) *err = std::string(#expr ": ") + hipGetErrorString(e_); \
            return -1;                                                       \
        }                                                                    \
    } while (0)

// CUs of the current device (per device: contexts on different GPUs share the process)
inline uint32_t num_cus() {
    constexpr int kMaxDev = 64;
    static std::atomic<uint32_t> cus[kMaxDev] = {};  // contexts on several threads may launch at once
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return 256;
    uint32_t c = cus[dev].load(std::memory_order_relaxed);
    if (!c) {
        hipDeviceProp_t p;
        c = (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? (uint32_t)p.multiProcessorCount
                                                                                       : 256u;
        cus[dev].store(c, std::memory_order_relaxed);
    }
    return c;
}

// workgroups of `kernel` that one CU holds at once (registers / LDS of this instantiation); 0 when
// the query fails
template <class K>
inline int occupancy(K kernel, int bs, size_t lds) {
    int per_cu = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, bs, lds) == hipSuccess && per_cu >= 1 ? per_cu : 0;
}

// Grid of a grid-stride kernel: exactly the workgroups that are resident at once, so no workgroup
// waits for another to finish, capped by the work and by blocks_per_cu when set. *occ: the
// occupancy before that cap.
template <class K>
inline int grid_resident(K kernel, int bs, size_t lds, uint64_t items, uint32_t blocks_per_cu, int* occ = nullptr) {
    int per_cu = std::max(1, occupancy(kernel, bs, lds));
    if (occ) *occ = per_cu;
    if (blocks_per_cu) per_cu = std::min<int>(per_cu, (int)blocks_per_cu);
    const uint64_t g = (items + bs - 1) / bs;
    return (int)std::max<uint64_t>(1, std::min<uint64_t>(g, (uint64_t)num_cus() * per_cu));
}

// The device scratch block of one call. The kernels of the call read and write it, so it is
// released only after the stream has run them: finish() waits for the stream and then frees, and a
// call that leaves early (a HIPCHK) waits for the whole device in the destructor.
class Scratch {
public:
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        if (!d) return;
        (void)hipDeviceSynchronize();
        (void)hipFree(d);
    }
    static int make(Scratch* s, size_t total, std::string* err) {
        void*& d = s->d;
        HIPCHK(hipMalloc(&d, total));
        return 0;
    }
    template <class T>
    T* at(size_t byte_off) const {
        return reinterpret_cast<T*>(static_cast<unsigned char*>(d) + byte_off);
    }
    // the end of a call whose launches all went out: a failed wait is "<what>: <hip error>"
    int finish(hipStream_t st, const char* what, std::string* err) {
        const hipError_t es = hipStreamSynchronize(st);
        (void)hipFree(d);
        d = nullptr;
        if (es == hipSuccess) return 0;
        if (err) *err = std::string(what) + ": " + hipGetErrorString(es);
        return -1;
    }

private:
    void* d = nullptr;
};

}  // namespace pg
