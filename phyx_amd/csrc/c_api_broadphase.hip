// c_api_broadphase.hip — extern "C" surface of the broadphase (see include/phyx_amd.h for the contract).
#include "handles.h"

extern "C" {

int phx_broadphase_create(phx_broadphase** out, int device)
{
    PHX_REQUIRE(out, "null out");
    *out = nullptr;
    PHX_TRY(phx::use_device(device));
    phx_broadphase* b = new (std::nothrow) phx_broadphase(device);
    PHX_REQUIRE(b, "out of host memory");
    int st = b->impl.init();
    if (st != PHX_OK) { delete b; return st; }
    *out = b;
    return PHX_OK;
}

void phx_broadphase_destroy(phx_broadphase* b) { delete b; }

int phx_broadphase_clear(phx_broadphase* b) { PHX_REQUIRE(b, "null handle"); return b->impl.clear(); }

int phx_broadphase_update(phx_broadphase* b, const phx_rigid_body* bodies, int32_t n, uint32_t* new_pairs, int32_t cap, int32_t* count)
{
    PHX_REQUIRE(b, "null handle");
    return b->impl.update_host(bodies, n, new_pairs, cap, count);
}

int phx_broadphase_update_device(phx_broadphase* b, const void* d_bodies, int32_t n)
{
    PHX_REQUIRE(b, "null handle");
    return b->impl.update_device(static_cast<const phx_rigid_body*>(d_bodies), n);
}

int phx_broadphase_get_sorted(phx_broadphase* b, phx_sort_entry* sorted, phx_broadphase_entry* entries, int32_t cap)
{
    PHX_REQUIRE(b, "null handle");
    return b->impl.get_sorted(sorted, entries, cap);
}

int phx_broadphase_get_new_pairs(phx_broadphase* b, uint32_t* new_pairs, int32_t cap, int32_t* count)
{
    PHX_REQUIRE(b, "null handle");
    return b->impl.get_new_pairs(new_pairs, cap, count);
}

int phx_broadphase_erase_pairs(phx_broadphase* b, const uint32_t* pairs, int32_t count)
{
    PHX_REQUIRE(b, "null handle");
    return b->impl.erase_pairs(pairs, count);
}

int phx_broadphase_get_stats(phx_broadphase* b, phx_broadphase_stats* out)
{
    PHX_REQUIRE(b, "null handle");
    return b->impl.get_stats(out);
}

} // extern "C"
