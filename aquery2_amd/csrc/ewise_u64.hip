// ewise_u64.hip -- the aqg_ewise and aqg_grouped_ewise kernels whose arithmetic runs in uint64_t (see ewise_impl.hpp)
#include "ewise_impl.hpp"
template int aqgew::dispatch_ot<uint64_t>(aqg_ctx*, int, int, int, int, const void*, int, const void*, void*, uint32_t, int);
template int aqgew::dispatch_got<uint64_t>(aqg_ctx*, int, int, int, int, const void*, int, const void*, const uint32_t*, void*, uint32_t, int);
