// What the audit HIP sources (reach.hip, closure.hip, groups.hip, paths.hip, classes.hip, zones.hip,
// dominators.hip, cut.hip, observed.hip, cost.hip) share on the host side of a launch, on top of hiputil.hpp: the section layout of a scratch block,
// the run grid of a kernel whose workgroups each take one contiguous run of work items, and the
// opt-in to more than 48 KiB of dynamic LDS. HIP only: no host .cpp file and not device.hip.
#pragma once
#include <vector>

#include "hiputil.hpp"

namespace pg {

// ---- a scratch block as a row of sections, each starting 16-B aligned ----------------------------
// The kernels store 16-B vectors into sections, so the alignment is not a nicety. Which contiguous
// run of sections the host fills and copies in is the caller's business.
template <size_t N>
struct Layout {
    size_t off[N], total;
    // section i in the device block
    template <class T>
    T* at(const Scratch& blk, size_t i) const {
        return blk.at<T>(off[i]);
    }
    // section i in a host image that starts at section `first`; n values at p copied there
    template <class T>
    T* in(std::vector<unsigned char>& h, size_t first, size_t i) const {
        return reinterpret_cast<T*>(h.data() + (off[i] - off[first]));
    }
    template <class T>
    void put(std::vector<unsigned char>& h, size_t first, size_t i, const T* p, size_t n) const {
        std::copy_n(p, n, in<T>(h, first, i));
    }
    template <class T>
    void put(std::vector<unsigned char>& h, size_t first, size_t i, const std::vector<T>& v) const {
        put(h, first, i, v.data(), v.size());
    }
};
template <size_t N>
constexpr Layout<N> lay_out(const size_t (&bytes)[N]) {
    Layout<N> l{};
    for (size_t i = 0; i < N; i++) {
        l.off[i] = (l.total + 15u) & ~(size_t)15u;
        l.total = l.off[i] + bytes[i];
    }
    return l;
}
constexpr auto kLay = lay_out({4, 16, 0, 8, 17, 1});
static_assert(kLay.off[0] == 0 && kLay.off[1] == 16 && kLay.off[2] == 32, "a section starts at the next multiple of 16");
static_assert(kLay.off[3] == 32, "a zero-size section takes no room and leaves the next one aligned");
static_assert(kLay.off[4] == 48 && kLay.off[5] == 80 && kLay.total == 81, "total ends with the last section, unpadded");
static_assert(lay_out({4, 16, 0, 8}).total == 40, "[0,4) [16,32) [32,32) [32,40)");

// ---- one contiguous run of work items per resident workgroup -----------------------------------------
// Workgroup b of `groups` takes items [b * per, min((b + 1) * per, items)). 64-bit arithmetic: a
// caller narrows to the width its shape struct has.
struct Runs {
    uint64_t per, groups;
};
// (items = 0 gives {0, 0}: no caller launches then)
constexpr Runs runs_of(uint64_t items, uint64_t grid) {
    const uint64_t per = (items + grid - 1) / grid;
    return Runs{per, per ? (items + per - 1) / per : 0};
}
template <class K>
inline Runs run_grid(K kernel, int bs, size_t lds, uint64_t items, uint32_t blocks_per_cu) {
    const int grid = grid_resident(kernel, bs, lds, items * (uint64_t)bs, blocks_per_cu);
    (void)hipGetLastError();  // (a failed occupancy query is answered by grid_resident's fall-back)
    return runs_of(items, (uint64_t)grid);
}
constexpr bool runs_are(uint64_t items, uint64_t grid, uint64_t per, uint64_t groups) {
    return runs_of(items, grid).per == per && runs_of(items, grid).groups == groups;
}
constexpr uint64_t kGrid = 1024, kBig = ((uint64_t)1 << 32) + 5;  // (of the checks)
static_assert(runs_are(0, kGrid, 0, 0) && runs_are(1, kGrid, 1, 1), "nothing; one item, one workgroup");
static_assert(runs_are(kGrid - 1, kGrid, 1, kGrid - 1) && runs_are(kGrid, kGrid, 1, kGrid), "up to one item each");
static_assert(runs_are(kGrid + 1, kGrid, 2, kGrid / 2 + 1), "runs of two: the groups shrink to those with work");
static_assert(runs_are(kBig, kGrid, ((uint64_t)1 << 22) + 1, kGrid), "no 32-bit wrap above 2^32 items");

// ---- more than 48 KiB of dynamic LDS: the kernel has to be told; the caller judges a failure ---------------
template <class K>
inline hipError_t allow_dynamic_lds(K kernel, size_t bytes) {
    if (bytes <= 48u * 1024u) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace pg
