// Test-only probes (include/cmdg.h): the shared-reciprocal quotient of exact_quotient.h next to the
// division, and the dry law's pointwise functions evaluated point by point -- on the device by one
// thread per point, on the host by the same text (where quot is the division).  No handle, no grid.
#include "../../include/cmdg.h"
#include "physics_atmos.h"

namespace cmdg {

__global__ void k_probe_quot(const double *a, const double *b, double *q_quot, double *q_div, int64_t n)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    q_quot[i] = quot(a[i], quot_pair(b[i]));
    q_div[i] = a[i] / b[i];
}

using ProbeLaw = DryAtmos<true, true, true, false, false, 0, true>;  // Held-Suarez at N = 4 (shared reciprocals)
static constexpr int PROBE_NOUT = 15 + 5 + 5 + ProbeLaw::NGRAD;
static_assert(ProbeLaw::NAUX == 17 && PROBE_NOUT == 33, "cmdg_probe_dry_atmos_pointwise documents 17 and 33");

__host__ __device__ inline void probe_point(const ProbeLaw::Params &m, const double *Q, const double *aux,
                                            const double *nrm, const double *der, double *out)
{
    double F[15], ws[5], S[5], G[ProbeLaw::NGRAD];
    ProbeLaw::flux_first_order(m, F, Q, aux, 0.0, DIR_EVERY);
    ProbeLaw::wavespeed(m, ws, nrm, Q, aux, 0.0, DIR_EVERY);
    ProbeLaw::source(m, S, Q, nullptr, aux, der, 0.0, DIR_EVERY);
    ProbeLaw::gradient_argument(m, G, Q, aux, 0.0);
    int o = 0;
    for (int i = 0; i < 15; ++i) out[o++] = F[i];
    for (int i = 0; i < 5; ++i) out[o++] = ws[i];
    for (int i = 0; i < 5; ++i) out[o++] = S[i];
    for (int i = 0; i < ProbeLaw::NGRAD; ++i) out[o++] = G[i];
}

__global__ void k_probe_dry_atmos(ProbeLaw::Params m, const double *Q, const double *aux, const double *nrm,
                                  const double *der, double *out, int64_t npts)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= npts) return;
    double q[5], a[ProbeLaw::NAUX], o[PROBE_NOUT];
    for (int s = 0; s < 5; ++s) q[s] = Q[5 * i + s];
    for (int s = 0; s < ProbeLaw::NAUX; ++s) a[s] = aux[ProbeLaw::NAUX * i + s];
    probe_point(m, q, a, nrm + 3 * i, der + 2 * i, o);
    for (int s = 0; s < PROBE_NOUT; ++s) out[PROBE_NOUT * i + s] = o[s];
}

static int probe_launched()
{
    hipError_t r = hipGetLastError();
    if (r == hipSuccess) r = hipDeviceSynchronize();
    return r == hipSuccess ? CMDG_OK : CMDG_ERR_HIP;
}

}  // namespace cmdg

using namespace cmdg;

extern "C" {

int cmdg_probe_quot(const double *a, const double *b, double *q_quot, double *q_div, int64_t n)
{
    if (!a || !b || !q_quot || !q_div || n < 0 || n > (int64_t(1) << 30)) return CMDG_ERR_INVALID;
    if (n == 0) return CMDG_OK;
    k_probe_quot<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(a, b, q_quot, q_div, n);
    return probe_launched();
}

int cmdg_probe_dry_atmos_pointwise(const int32_t *iparam, const double *dparam, int32_t where, const double *Q,
                                   const double *aux, const double *nrm, const double *der, double *out,
                                   int64_t npts)
{
    if (!iparam || !dparam || !Q || !aux || !nrm || !der || !out || npts < 0 || npts > (int64_t(1) << 24) ||
        (where != 0 && where != 1))
        return CMDG_ERR_INVALID;
    if (!(iparam[0] != 0 && iparam[1] != 0 && iparam[4] != 0 && iparam[14] == 0 && atmos_ntracers(iparam) == 0))
        return CMDG_ERR_UNSUPPORTED;
    ProbeLaw::Params m;
    ProbeLaw::make_params(m, iparam, dparam);
    if (npts == 0) return CMDG_OK;
    if (where == 0) {
        for (int64_t i = 0; i < npts; ++i)
            probe_point(m, Q + 5 * i, aux + ProbeLaw::NAUX * i, nrm + 3 * i, der + 2 * i, out + PROBE_NOUT * i);
        return CMDG_OK;
    }
    k_probe_dry_atmos<<<dim3((unsigned)((npts + 127) / 128)), dim3(128)>>>(m, Q, aux, nrm, der, out, npts);
    return probe_launched();
}

}  // extern "C"
