// Range guard of the split-fp16 arithmetic: one flag per process, in two places.  Kernels raise it (guard_raise,
// ojf_common.h) when a value that a later layer would split leaves the fp16 range (or is NaN): in a device-resident
// block {flag, skipped integrate calls, pointer to the mirror} - what ojf_integrate* test before they touch a volume, so
// that a frame whose net tripped the guard (and every frame after it, until the host has dealt with it) is NOT fused -
// and in a host-mapped mirror, which the host polls without synchronising (ojf_net_forward, ojf_trainer_forward) or after a
// stream synchronise (ojf_net_check).  No traffic unless it fires.  The fusion net, the training executor, the segmentation
// convolutions and the integrate kernels all see THIS flag: its state is defined here and nowhere else.
#include "ojf_common.h"

namespace ojf {

static volatile int *g_ovf_host = nullptr;
static int *g_ovf_dev = nullptr;  // device block: [0] flag, [1] integrate calls skipped, [2..3] device address of the mirror

int *overflow_flag()
{
    if (!g_ovf_dev) {
        void *h = nullptr, *hd = nullptr, *d = nullptr;
        if (hipHostMalloc(&h, sizeof(int), hipHostMallocMapped) != hipSuccess) return nullptr;
        *static_cast<int *>(h) = 0;
        if (hipHostGetDevicePointer(&hd, h, 0) != hipSuccess) return nullptr;
        if (hipMalloc(&d, 16) != hipSuccess) return nullptr;
        struct { int flag, skipped; void *mirror; } init{0, 0, hd};
        static_assert(sizeof(init) == 16, "guard block layout");
        if (hipMemcpy(d, &init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        g_ovf_host = static_cast<volatile int *>(h);
        g_ovf_dev = static_cast<int *>(d);
    }
    return g_ovf_dev;
}

int *range_flag_device() { return overflow_flag(); }  // ojf_seg.hip
const int *range_guard_if_any() { return g_ovf_dev; }  // ojf_integrate*.hip: NULL while no split-fp16 kernel ever got the flag

int guard_take(int *skipped, bool clear)
{
    if (!g_ovf_host || !*g_ovf_host) {
        if (skipped) *skipped = 0;
        return 0;
    }
    const int what = *g_ovf_host;
    int blk[2] = {what, 0};
    (void)hipMemcpy(blk, g_ovf_dev, sizeof(blk), hipMemcpyDeviceToHost);
    if (skipped) *skipped = blk[1];
    if (clear) {
        (void)hipMemset(g_ovf_dev, 0, 2 * sizeof(int));
        (void)hipStreamSynchronize(nullptr);  // (non-blocking streams do not order against the null stream's fill: see ojf_net.hip alloc_planes)
        *g_ovf_host = 0;
    }
    return what;
}

static const char *kChainStuckMsg =
    "fusion net: dense_chain_kernel gave up waiting for a neighbouring tile (internal error: the results of this forward pass are invalid)";
static const char *kOverflowMsg =
    "split-fp16 arithmetic: an activation or input left the fp16 range (|x| > 65504 or NaN); results since the last "
    "ojf_net_check are invalid - use ojf_net_set_arithmetic(OJF_ARITH_F32) for this network";

int guard_fail(int what) { return fail(what == 2 ? kChainStuckMsg : kOverflowMsg); }

int guard_refusal()
{
    const int what = g_ovf_host ? *g_ovf_host : 0;
    return what ? guard_fail(what) : 0;
}

}  // namespace ojf

OJF_API int ojf_net_check(ojf_stream_t stream)
{
    using namespace ojf;
    OJF_HIP(hipStreamSynchronize(as_stream(stream)));
    if (const int what = guard_take(nullptr, true)) return guard_fail(what);
    return 0;
}

OJF_API int ojf_guard_poll(void) { return ojf::g_ovf_host ? *ojf::g_ovf_host : 0; }

OJF_API int ojf_guard_status(ojf_stream_t stream, int *flag, int *skipped)
{
    using namespace ojf;
    OJF_HIP(hipStreamSynchronize(as_stream(stream)));
    const int what = guard_take(skipped, false);
    if (flag) *flag = what;
    return 0;
}
