// dev_str.h -- the pointer and length of string i of a StrView, for the kernels that take one string per lane.  Device-only.
// (wave.h's load_str is the wavefront form with a validity mask, lev_wide.hip's wide_str the one over 16- and 32-bit symbols.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave.h"

namespace ta {

__device__ __forceinline__ void dev_str(const StrView &s, uint32_t i, const uint8_t *&p, uint64_t &len) {
    if (s.off) {
        const uint64_t o0 = s.off[i], o1 = s.off[i + 1];
        p = s.blob + o0;
        len = o1 - o0;
    } else {
        p = s.blob + (uint64_t)i * s.stride;
        len = s.len;
    }
}

}  // namespace ta
