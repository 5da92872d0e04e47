// Export of include/features/restore_pool/rpx_restore_pool.h: the update launch of the restoring pool.
#include "host.h"
#include "../../include/features/restore_pool/rpx_restore_pool.h"
#include "restore_pool_kernels.h"

static_assert(RPX_KNOWN_STRIDE == kRpxKnownStride && RPX_FLAGS_WORD == kRpxFlagsWord && RPX_KNOWN == kRpxKnown,
              "rpx_restore_pool.h and restore_pool_kernels.h disagree");
static_assert(RPX_FLAGS_WORD < DDIMX_POOL_SLOT_WORDS, "the flags word lies inside the pool's slot-table row");

extern "C" {

int rpx_pool_update(float* xt, const float* eps, float* x0, float* hist, const float* y, const float* mask, const float* arena,
                    const float* known, const int* slots, int n_slots, int max_steps, long long per_sample, void* stream) {
    if (!xt || !eps || !x0 || !hist || !y || !mask || !arena || !known || !slots) return fail("rpx_pool_update: null argument");
    if (n_slots < 1 || n_slots > 65535) return fail("rpx_pool_update: n_slots = %d (1..65535)", n_slots);
    if (max_steps < 1) return fail("rpx_pool_update: max_steps = %d must be positive", max_steps);
    CHK(sample_shape("rpx_pool_update", n_slots, per_sample));
    CHK(noise_range("rpx_pool_update", n_slots, per_sample, 0));  // a slot's sample index is a word of the slot table: any value fits
    HIPCHK(rpx_pool_update_launch(xt, eps, x0, hist, y, mask, arena, known, slots, n_slots, max_steps, per_sample, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
