// ewise_f32.hip -- the aqg_ewise and aqg_grouped_ewise kernels whose arithmetic runs in float (see ewise_impl.hpp)
#include "ewise_impl.hpp"
template int aqgew::dispatch_ot<float>(aqg_ctx*, int, int, int, int, const void*, int, const void*, void*, uint32_t, int);
template int aqgew::dispatch_got<float>(aqg_ctx*, int, int, int, int, const void*, int, const void*, const uint32_t*, void*, uint32_t, int);
