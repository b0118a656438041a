// The device arrays of a plan: see plan_core.hpp (the arithmetic is plan_arith.cc).
#include "plan_core.hpp"

hipError_t MiPlanCore::allocate(uint32_t n_alloc_max, size_t e_bytes_max, void *d_desc_block)
{
    cap_alloc   = n_alloc_max;
    cap_e_bytes = e_bytes_max ? e_bytes_max : 64;
    desc_views  = d_desc_block != nullptr;
    hipError_t e;
    if (desc_views) {
        d_allocs   = (mi_lte_pdsch_alloc *)d_desc_block;
        d_e_off    = (uint32_t *)(d_allocs + cap_alloc);
        d_cb_alloc = d_e_off + cap_alloc;
    } else if ((e = hipMalloc((void **)&d_allocs, sizeof(mi_lte_pdsch_alloc) * cap_alloc)) != hipSuccess || (e = hipMalloc((void **)&d_e_off, sizeof(uint32_t) * cap_alloc)) != hipSuccess ||
               (e = hipMalloc((void **)&d_cb_alloc, sizeof(uint32_t) * cap_alloc)) != hipSuccess)
        return e;
    if ((e = hipMalloc((void **)&d_e_len, sizeof(uint32_t) * cap_alloc)) != hipSuccess) return e;
    return hipMalloc((void **)&d_e, cap_e_bytes);
}

void MiPlanCore::release()
{
    if (!desc_views)
        for (void *p : {(void *)d_allocs, (void *)d_e_off, (void *)d_cb_alloc}) (void)hipFree(p);
    (void)hipFree(d_e_len);
    (void)hipFree(d_e);
    mi_multi_cache_free(&multi);
}
