// launch.h -- the one place that dispatches on the ring degree and launches a kernel (host side; included by the
// four .hip files only).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace seamd {

// f(std::integral_constant<int, LOGN>{}) for the degree 2^logn of the context; inside a generic lambda,
// `constexpr int L = decltype(l)::value` names the template argument of the kernel.
template <class F>
static inline hipError_t for_logn(unsigned logn, F &&f)
{
    switch (logn)
    {
        case 10: return f(std::integral_constant<int, 10>{});
        case 11: return f(std::integral_constant<int, 11>{});
        case 12: return f(std::integral_constant<int, 12>{});
        case 13: return f(std::integral_constant<int, 13>{});
        case 14: return f(std::integral_constant<int, 14>{});
        default: return hipErrorInvalidValue;
    }
}

// One launch.  A launch that asks for dynamic LDS raises the kernel's limit to it first (every time: the
// attribute belongs to the kernel, and the sizes of one kernel differ between calls).
template <class... KArgs, class... Args>
static inline hipError_t launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st,
                                Args &&...args)
{
    if (lds_bytes != 0)
        (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, st, args...);
    return hipGetLastError();
}

// compute units of the device as the grid arithmetic uses them: 0 (not known) counts as an MI355X
static inline unsigned cus_or_default(unsigned num_cus) { return num_cus ? num_cus : 256u; }

}  // namespace seamd
