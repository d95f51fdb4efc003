// k_smooth_loo_wide.hip -- loo_back_kernel for responses of five to eight columns run as ONE filter (a translation unit of its own for build time)
#define SSDE_LOO_WIDE_TU 1
#define SSDE_DENSE_NOUNROLL 1
#include "k_smooth_loo.hip"
