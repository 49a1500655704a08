/*
 * mfm_runrs_view.hip - the plan kernel of the burst resampler's view entries (mfm_runrs_process_view_device,
 * mfm_runrs_process_bits_view_device): a resampler sized to one local route of the run router (mfm_runroute_create_local) reads
 * the gate's payload in place.  It is rr_plan_kernel (mfm_runrs.hip) with one difference, and shares its body
 * (mfm_runrs_kernels.h, rr_plan_body): a run's payload range is checked against *d_payload_elems, how much payload exists, where
 * rr_plan_kernel checks it against the totals' elements, which here are only the route's load.  The scan, FIR, DC, bits and state
 * kernels behind it are the ones the plain entries queue.  An object of its own, as mfm_runrs_dc.hip is, so that every other
 * object keeps the kernels it had.
 */
#include <hip/hip_runtime.h>

#include "../../include/multifm_hip.h"

#include "mfm_numerics.h"
#include "mfm_runrs.h"
#include "mfm_runrs_kernels.h"

namespace {

__global__ __launch_bounds__(256) void rrv_plan_kernel(const RrCall A, const uint64_t *payload_elems)
{
    rr_plan_body<true>(A, payload_elems);
}

} /* namespace */

extern "C" __attribute__((visibility("hidden"))) int mfm_internal_runrs_view_plan_launch(const void *call, const uint64_t *d_payload_elems,
                                                                                        uint32_t cap_runs, hipStream_t s)
{
    const RrCall &A = *static_cast<const RrCall *>(call);
    /* run count and flags are read on the device: sized from the capacity, as rr_plan_kernel's launch */
    hipLaunchKernelGGL(rrv_plan_kernel, dim3((cap_runs + 255u) / 256u), dim3(256), 0, s, A, d_payload_elems);
    return hipPeekAtLastError() == hipSuccess ? MFM_OK : MFM_E_DEVICE;
}
