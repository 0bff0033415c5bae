// Interpolation of DG states onto box and latitude-longitude grids: interpolate_local!,
// project_cubed_sphere! and the device half of accumulate_interpolated_data!
// (src/Numerics/Mesh/Interpolation.jl:397-570, :1332-1414, :1548-1561).
//
// The reference gives one work-group of Nq2 x Nq3 threads to an element and walks the element's
// points one at a time, three barriers per point.  Here a work-group owns a chunk of at most NT
// points of ONE element (the host cuts every element's point list into such chunks at create, so
// elements without points cost nothing and a polar element with thousands of points spreads over
// many work-groups).  The group stages the element's states into LDS with coalesced loads -- all of
// them when Np nstate 8 B fits LDS_BYTES, else chunks of states -- and every lane owns one point: it
// builds its 2 Nq_h + Nq_v one-dimensional Lagrange weights in registers (barycentric form,
// normalised per direction; a xi within 4 eps of a node gives the unit vector of that node, so no
// quotient of infinities is formed) and walks the element in LDS.  All lanes read the same LDS
// address at the same time: a broadcast, free of bank conflicts.  The sums are fma chains
// (this file's arithmetic is its own: the reference's order is restated by the tests, and the
// kernel is held to it within 1e-12).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "interpolation.h"
#include "engine_base.h"
#include "with_constant.h"

namespace cmdg {

namespace {
constexpr int NT = 128;            // threads per work-group = points per chunk
constexpr int LDS_BYTES = 32768;   // staged states per pass: N = 7 (Np = 512) takes 8 states
constexpr int QMIN = 2, QMAX = 8;  // compiled points per direction
constexpr double XI_SLACK = 1e-10;

struct Work {
    int32_t e, p0, n, pad;  // element, first point, points (1..NT)
};
struct Nodes {
    double m[2][QMAX], wb[2][QMAX];  // [0] horizontal, [1] vertical: LGL nodes, barycentric weights
};

template <int N>
__device__ __forceinline__ void lagrange(double xi, const double *m, const double *wb, double *l)
{
    constexpr double toler = 4 * 2.220446049250313e-16;
    int hit = -1;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double d = xi - m[i];
        const bool on = fabs(d) < toler;
        const double t = wb[i] / d;
        l[i] = t;
        if (on)
            hit = i;
        else
            s += t;
    }
    const double inv = 1.0 / s;
#pragma unroll
    for (int i = 0; i < N; ++i) l[i] = hit >= 0 ? (i == hit ? 1.0 : 0.0) : l[i] * inv;
}

template <int QH, int QV>
__global__ __launch_bounds__(NT) void k_interpolate(const Work *__restrict__ work, const double *__restrict__ xi1,
                                                    const double *__restrict__ xi2, const double *__restrict__ xi3,
                                                    const double *__restrict__ Q, double *__restrict__ v, int nstate,
                                                    int nsc, int64_t npoints, Nodes nd)
{
    extern __shared__ double sQ[];
    constexpr int NP = QH * QH * QV;
    const Work w = work[blockIdx.x];
    const int tid = threadIdx.x;
    const bool active = tid < w.n;
    const int64_t p = (int64_t)w.p0 + tid;
    double l1[QH], l2[QH], l3[QV];
    if (active) {
        lagrange<QH>(xi1[p], nd.m[0], nd.wb[0], l1);
        lagrange<QH>(xi2[p], nd.m[0], nd.wb[0], l2);
        lagrange<QV>(xi3[p], nd.m[1], nd.wb[1], l3);
    }
    const double *Qe = Q + (int64_t)w.e * nstate * NP;
    for (int s0 = 0; s0 < nstate; s0 += nsc) {
        const int ns = min(nsc, nstate - s0);
        if (s0) __syncthreads();
        const double *src = Qe + (int64_t)s0 * NP;  // states s0 .. s0 + ns - 1 of the element: contiguous
        for (int i = tid; i < ns * NP; i += NT) sQ[i] = src[i];
        __syncthreads();
        if (!active) continue;
        for (int s = 0; s < ns; ++s) {
            const double *q = sQ + s * NP;
            double a3 = 0.0;
#pragma unroll
            for (int k = 0; k < QV; ++k) {
                double a2 = 0.0;
#pragma unroll
                for (int j = 0; j < QH; ++j) {
                    double a1 = 0.0;
#pragma unroll
                    for (int i = 0; i < QH; ++i) a1 = fma(l1[i], q[i + QH * (j + QH * k)], a1);
                    a2 = fma(l2[j], a1, a2);
                }
                a3 = fma(l3[k], a2, a3);
            }
            v[p + (int64_t)(s0 + s) * npoints] = a3;
        }
    }
}

// project_cubed_sphere! at one point (:1332-1414): the unit vectors of the point's latitude and longitude
struct LatLong {
    double cl, sl, co, so;
    __device__ LatLong(double lat_deg, double long_deg)
    {
        const double deg2rad = M_PI / 180.0;
        const double la = lat_deg * deg2rad, lo = long_deg * deg2rad;
        cl = cos(la), sl = sin(la), co = cos(lo), so = sin(lo);
    }
    // Cartesian (x, y, z) -> components along longitude, latitude, radius
    __device__ __forceinline__ void project(double x, double y, double z, double &vlon, double &vlat,
                                            double &vrad) const
    {
        vrad = x * cl * co + y * cl * so + z * sl;
        vlat = -x * sl * co - y * sl * so + z * cl;
        vlon = -x * so + y * co;
    }
};

__global__ void k_project(double *__restrict__ v, const int32_t *__restrict__ ilong, const int32_t *__restrict__ ilat,
                          const double *__restrict__ long_grd, const double *__restrict__ lat_grd, int64_t npoints,
                          int cu, int cv, int cw)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npoints) return;
    const LatLong ll(lat_grd[ilat[p] - 1], long_grd[ilong[p] - 1]);
    double vlon, vlat, vrad;
    ll.project(v[p + cu * npoints], v[p + cv * npoints], v[p + cw * npoints], vlon, vlat, vrad);
    v[p + cu * npoints] = vlon;
    v[p + cv * npoints] = vlat;
    v[p + cw * npoints] = vrad;
}

// The finishing pass of the AtmosGCMDefault group (atmos_gcm_default.jl:375-379, :150-165): vG (14,
// npoints) the interpolated nodal array (kernels.h GCM_NCOL), vB (3, npoints) the interpolated
// VorticityModel tendency.  Projects rho u, Omega and Omega_bl, forms u, v, w = rho u_i / rho_i and et =
// rho e_i / rho_i and stores u, v, w, rho, temp, pres, thd, et, ei, ht, hi, vort, vort2 as k_scatter stores.
constexpr int GCM_NIN = 14, GCM_NOUT = 13;
__global__ void k_gcm_finish(double *__restrict__ fiv, const double *__restrict__ vG, const double *__restrict__ vB,
                             const int32_t *__restrict__ i1, const int32_t *__restrict__ i2,
                             const int32_t *__restrict__ i3, const double *__restrict__ long_grd,
                             const double *__restrict__ lat_grd, int64_t npoints, int64_t n1, int64_t n2, int64_t n3)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npoints) return;
    const LatLong ll(lat_grd[i2[p] - 1], long_grd[i1[p] - 1]);
    double g[GCM_NIN];
#pragma unroll
    for (int s = 0; s < GCM_NIN; ++s) g[s] = vG[p + npoints * s];
    double mlon, mlat, mrad, olon, olat, orad, blon, blat, brad;
    ll.project(g[1], g[2], g[3], mlon, mlat, mrad);
    ll.project(g[11], g[12], g[13], olon, olat, orad);
    ll.project(vB[p], vB[p + npoints], vB[p + 2 * npoints], blon, blat, brad);
    const double rho = g[0];
    const double out[GCM_NOUT] = {mlon / rho, mlat / rho, mrad / rho, rho,  g[5], g[6], g[7],
                                  g[4] / rho, g[8],       g[9],       g[10], orad, brad};
    const int64_t at = (i1[p] - 1) + n1 * ((i2[p] - 1) + n2 * (int64_t)(i3[p] - 1));
    const int64_t ntot = n1 * n2 * n3;
#pragma unroll
    for (int s = 0; s < GCM_NOUT; ++s) fiv[at + ntot * s] = out[s];
}

__global__ void k_scatter(double *__restrict__ fiv, const double *__restrict__ v, const int32_t *__restrict__ i1,
                          const int32_t *__restrict__ i2, const int32_t *__restrict__ i3, int64_t npoints,
                          int64_t n1, int64_t n2, int64_t n3, int nstate)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npoints) return;
    const int64_t at = (i1[p] - 1) + n1 * ((i2[p] - 1) + n2 * (int64_t)(i3[p] - 1));
    const int64_t ntot = n1 * n2 * n3;
    for (int s = 0; s < nstate; ++s) fiv[at + ntot * s] = v[p + npoints * s];
}

using InterpKernel = void (*)(const Work *, const double *, const double *, const double *, const double *, double *,
                              int, int, int64_t, Nodes);
// NULL: an order that is not compiled in
InterpKernel pick(int qh, int qv)
{
    InterpKernel k = nullptr;
    with_constant<QMIN, QMAX>(qh, [&](auto h) {
        with_constant<QMIN, QMAX>(qv, [&](auto v) { k = k_interpolate<h(), v()>; });
    });
    return k;
}

template <class T>
bool upload(DevBuf<T> &dst, const T *src, size_t n)
{
    if (n == 0) return true;
    if (dst.alloc(n) != hipSuccess) return false;
    return hipMemcpy(dst, src, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
}

int finish(hipStream_t st, bool wait, const char *what, std::string &err)
{
    hipError_t r = hipGetLastError();
    if (r == hipSuccess && wait) r = hipStreamSynchronize(st);
    if (r != hipSuccess) {
        err = std::string(what) + ": " + hipGetErrorString(r);
        return CMDG_ERR_HIP;
    }
    return CMDG_OK;
}
}  // namespace

struct InterpObj {
    int dev = 0;
    int QH = 0, QV = 0, Np = 0;
    int64_t nelem = 0, npoints = 0, n1 = 0, n2 = 0, n3 = 0;
    Nodes nd{};
    InterpKernel kernel = nullptr;
    DevBuf<double> xi[3];
    DevBuf<int32_t> idx[3];
    DevBuf<double> lat, lon;
    DevBuf<Work> work;
    int64_t nwork = 0;
};

int interp_device(const InterpObj *o) { return o->dev; }

void interp_destroy(InterpObj *o) { delete o; }

int interp_create(const cmdg_interp_desc *d, InterpObj **out, std::string &err)
{
    *out = nullptr;
    auto invalid = [&](const std::string &m) {
        err = "cmdg_interp_create: " + m;
        return CMDG_ERR_INVALID;
    };
    if (d->nelem < 0 || d->npoints < 0 || d->n1 < 1 || d->n2 < 1 || d->n3 < 1) return invalid("negative size");
    // no offset and no xi tables: an object that is only projected and scattered (a root that holds
    // the gathered index triples of every rank); Nq, nelem and the nodes are then not read
    const bool tables_only = !d->offset && !d->xi1 && !d->xi2 && !d->xi3;
    if (!tables_only && (!d->offset || !d->xi_nodes[0] || !d->xi_nodes[1] || !d->xi_nodes[2]))
        return invalid("missing offset or nodes");
    if (d->npoints > 0 && (!d->i1 || !d->i2 || !d->i3 || (!tables_only && (!d->xi1 || !d->xi2 || !d->xi3))))
        return invalid("missing point tables");
    if ((d->lat_grd == nullptr) != (d->long_grd == nullptr)) return invalid("lat_grd and long_grd go together");
    if (!tables_only) {
        if (d->Nq[0] != d->Nq[1]) {
            err = "cmdg_interp_create: one horizontal polynomial order only (Nq[0] == Nq[1])";
            return CMDG_ERR_UNSUPPORTED;
        }
        for (int k = 0; k < 3; ++k)
            if (d->Nq[k] < QMIN || d->Nq[k] > QMAX) {
                err = "cmdg_interp_create: compiled for 2 to 8 points per direction, got " + std::to_string(d->Nq[k]);
                return CMDG_ERR_UNSUPPORTED;
            }
    }
    if (d->npoints > INT32_MAX || (double)d->n1 * (double)d->n2 * (double)d->n3 > (double)INT32_MAX)
        return invalid("more than 2^31 - 1 points");
    // the point tables decide every address the kernels form: check them here, once
    if (!tables_only) {
        if (d->offset[0] != 0) return invalid("offset does not start at 0");
        for (int64_t e = 0; e < d->nelem; ++e)
            if (d->offset[e + 1] < d->offset[e])
                return invalid("offset decreases at element " + std::to_string(e));
        if (d->offset[d->nelem] != d->npoints)
            return invalid("offset ends at " + std::to_string(d->offset[d->nelem]) + ", npoints is " +
                           std::to_string(d->npoints));
    }
    const double *xis[3] = {d->xi1, d->xi2, d->xi3};
    const int32_t *ids[3] = {d->i1, d->i2, d->i3};
    const int64_t ns[3] = {d->n1, d->n2, d->n3};
    for (int k = 0; k < 3; ++k)
        for (int64_t p = 0; p < d->npoints; ++p) {
            if (!tables_only && !(fabs(xis[k][p]) <= 1.0 + XI_SLACK))
                return invalid("xi" + std::to_string(k + 1) + " of point " + std::to_string(p) + " is " +
                               std::to_string(xis[k][p]) + ", outside [-1, 1]");
            if (ids[k][p] < 1 || ids[k][p] > ns[k])
                return invalid("index i" + std::to_string(k + 1) + " of point " + std::to_string(p) + " is " +
                               std::to_string(ids[k][p]) + ", outside 1.." + std::to_string(ns[k]));
        }
    InterpObj *o = new InterpObj;
    (void)hipGetDevice(&o->dev);
    o->npoints = d->npoints;
    o->n1 = d->n1, o->n2 = d->n2, o->n3 = d->n3;
    std::vector<Work> work;
    if (!tables_only) {
        o->QH = d->Nq[0];
        o->QV = d->Nq[2];
        o->Np = o->QH * o->QH * o->QV;
        o->nelem = d->nelem;
        o->kernel = pick(o->QH, o->QV);
        if (!o->kernel) {
            delete o;
            err = "cmdg_interp_create: compiled for 2 to 8 points per direction";
            return CMDG_ERR_UNSUPPORTED;
        }
        for (int hv = 0; hv < 2; ++hv) {  // baryweights(r): wb_i = 1 / prod_{j != i} (r_i - r_j)
            const double *m = d->xi_nodes[hv ? 2 : 0];
            const int n = hv ? o->QV : o->QH;
            for (int i = 0; i < QMAX; ++i) o->nd.m[hv][i] = o->nd.wb[hv][i] = 0.0;
            for (int i = 0; i < n; ++i) {
                double w = 1.0;
                for (int j = 0; j < n; ++j)
                    if (j != i) w *= m[i] - m[j];
                o->nd.m[hv][i] = m[i];
                o->nd.wb[hv][i] = 1.0 / w;
            }
        }
        for (int i = 0; i < o->QH; ++i)
            if (d->xi_nodes[1][i] != d->xi_nodes[0][i]) {
                delete o;
                return invalid("the two horizontal directions have different nodes");
            }
        for (int64_t e = 0; e < d->nelem; ++e)
            for (int64_t p0 = d->offset[e]; p0 < d->offset[e + 1]; p0 += NT)
                work.push_back({(int32_t)e, (int32_t)p0, (int32_t)std::min<int64_t>(NT, d->offset[e + 1] - p0), 0});
    }
    o->nwork = (int64_t)work.size();
    bool ok = upload(o->work, work.data(), work.size());
    for (int k = 0; k < 3 && ok; ++k)
        ok = (tables_only || upload(o->xi[k], xis[k], (size_t)d->npoints)) && upload(o->idx[k], ids[k], (size_t)d->npoints);
    if (ok && d->lat_grd) ok = upload(o->lat, d->lat_grd, (size_t)d->n2) && upload(o->lon, d->long_grd, (size_t)d->n1);
    if (!ok) {
        (void)hipGetLastError();
        interp_destroy(o);
        err = "cmdg_interp_create: device allocation or copy failed";
        return CMDG_ERR_HIP;
    }
    *out = o;
    return CMDG_OK;
}

int interp_apply(const InterpObj *o, const double *Q, int nstate, int64_t nelemQ, double *v, hipStream_t st,
                 bool wait, std::string &err)
{
    if (!o->kernel) {
        err = "cmdg_interp_apply: the object was created without offset and xi tables (projection and scatter only)";
        return CMDG_ERR_INVALID;
    }
    if (nelemQ < o->nelem) {
        err = "cmdg_interp_apply: Q has " + std::to_string(nelemQ) + " elements, the point tables address " +
              std::to_string(o->nelem);
        return CMDG_ERR_INVALID;
    }
    if (o->nwork == 0) return CMDG_OK;
    const int nsc = std::max(1, std::min(nstate, LDS_BYTES / (o->Np * (int)sizeof(double))));
    const size_t lds = (size_t)nsc * o->Np * sizeof(double);
    hipLaunchKernelGGL(o->kernel, dim3((unsigned)o->nwork), dim3(NT), lds, st, o->work, o->xi[0], o->xi[1], o->xi[2],
                       Q, v, nstate, nsc, o->npoints, o->nd);
    return finish(st, wait, "cmdg_interp_apply", err);
}

int interp_project(const InterpObj *o, double *v, int nstate, const int32_t *uvwi, hipStream_t st, bool wait,
                   std::string &err)
{
    if (!o->lat) {
        err = "cmdg_interp_project: the object has no latitude-longitude grid (a brick)";
        return CMDG_ERR_INVALID;
    }
    for (int k = 0; k < 3; ++k)
        if (uvwi[k] < 1 || uvwi[k] > nstate) {
            err = "cmdg_interp_project: column " + std::to_string(uvwi[k]) + " is outside 1.." + std::to_string(nstate);
            return CMDG_ERR_INVALID;
        }
    if (uvwi[0] == uvwi[1] || uvwi[0] == uvwi[2] || uvwi[1] == uvwi[2]) {
        err = "cmdg_interp_project: a column is named twice";
        return CMDG_ERR_INVALID;
    }
    if (o->npoints == 0) return CMDG_OK;
    hipLaunchKernelGGL(k_project, dim3((unsigned)((o->npoints + 255) / 256)), dim3(256), 0, st, v, o->idx[0], o->idx[1],
                       o->lon, o->lat, o->npoints, uvwi[0] - 1, uvwi[1] - 1, uvwi[2] - 1);
    return finish(st, wait, "cmdg_interp_project", err);
}

int interp_scatter(const InterpObj *const *o, int n, const double *const *v, int nstate, double *fiv, hipStream_t st,
                   bool wait, std::string &err)
{
    for (int r = 0; r < n; ++r) {
        if (o[r]->n1 != o[0]->n1 || o[r]->n2 != o[0]->n2 || o[r]->n3 != o[0]->n3 || o[r]->dev != o[0]->dev) {
            err = "cmdg_interp_scatter: object " + std::to_string(r) + " has another output grid or device";
            return CMDG_ERR_INVALID;
        }
        if (o[r]->npoints > 0 && !v[r]) {
            err = "cmdg_interp_scatter: no array for object " + std::to_string(r);
            return CMDG_ERR_INVALID;
        }
    }
    for (int r = 0; r < n; ++r) {
        if (o[r]->npoints == 0) continue;
        hipLaunchKernelGGL(k_scatter, dim3((unsigned)((o[r]->npoints + 255) / 256)), dim3(256), 0, st, fiv, v[r],
                           o[r]->idx[0], o[r]->idx[1], o[r]->idx[2], o[r]->npoints, o[r]->n1, o[r]->n2, o[r]->n3, nstate);
    }
    return finish(st, wait, "cmdg_interp_scatter", err);
}

int interp_gcm_finish(const InterpObj *const *o, int n, const double *const *vG, const double *const *vB, double *fiv,
                      hipStream_t st, bool wait, std::string &err)
{
    for (int r = 0; r < n; ++r) {
        if (!o[r]->lat) {
            err = "cmdg_interp_gcm_finish: object " + std::to_string(r) + " has no latitude-longitude grid (a brick)";
            return CMDG_ERR_INVALID;
        }
        if (o[r]->n1 != o[0]->n1 || o[r]->n2 != o[0]->n2 || o[r]->n3 != o[0]->n3 || o[r]->dev != o[0]->dev) {
            err = "cmdg_interp_gcm_finish: object " + std::to_string(r) + " has another output grid or device";
            return CMDG_ERR_INVALID;
        }
        if (o[r]->npoints > 0 && (!vG[r] || !vB[r])) {
            err = "cmdg_interp_gcm_finish: no arrays for object " + std::to_string(r);
            return CMDG_ERR_INVALID;
        }
    }
    for (int r = 0; r < n; ++r) {
        if (o[r]->npoints == 0) continue;
        hipLaunchKernelGGL(k_gcm_finish, dim3((unsigned)((o[r]->npoints + 255) / 256)), dim3(256), 0, st, fiv, vG[r],
                           vB[r], o[r]->idx[0], o[r]->idx[1], o[r]->idx[2], o[r]->lon, o[r]->lat, o[r]->npoints,
                           o[r]->n1, o[r]->n2, o[r]->n3);
    }
    return finish(st, wait, "cmdg_interp_gcm_finish", err);
}

}  // namespace cmdg

// ---- the C entries ------------------------------------------------------------------------------
using namespace cmdg;

extern "C" {

int cmdg_interp_create(cmdg_handle h, const cmdg_interp_desc *d, cmdg_interp *out)
{
    if (!d || !out) return CMDG_ERR_INVALID;
    std::optional<DevGuard> guard_;
    if (h) guard_.emplace(h->eng);
    InterpObj *o = nullptr;
    std::string err;
    const int r = interp_create(d, &o, err);
    *out = reinterpret_cast<cmdg_interp>(o);
    return object_call_done(h, r, err);
}

int cmdg_interp_destroy(cmdg_handle h, cmdg_interp it)
{
    if (!it) return CMDG_ERR_INVALID;
    InterpObj *o = reinterpret_cast<InterpObj *>(it);
    std::optional<DevGuard> guard_;
    if (h) {
        guard_.emplace(h->eng);
        h->eng->synchronize();
    }
    ObjectDevice dev_(interp_device(o));
    (void)hipStreamSynchronize(nullptr);  // (calls without a handle have returned; see include/cmdg.h)
    interp_destroy(o);
    return CMDG_OK;
}

int cmdg_interp_apply(cmdg_handle h, cmdg_interp it, const double *Q, int32_t nstate, int64_t nelemQ, double *v)
{
    if (!it || !Q || !v || nstate < 1) return CMDG_ERR_INVALID;
    const InterpObj *o = reinterpret_cast<const InterpObj *>(it);
    std::optional<DevGuard> guard_;
    if (h) guard_.emplace(h->eng);
    std::string err;
    if (h && h->eng->dev != interp_device(o))
        return object_call_done(h, CMDG_ERR_INVALID, "cmdg_interp_apply: the object lives on another device than the handle");
    ObjectDevice dev_(interp_device(o));
    return object_call_done(h, interp_apply(o, Q, nstate, nelemQ, v, h ? h->eng->s_comp : nullptr, !h, err), err);
}

int cmdg_interp_project(cmdg_handle h, cmdg_interp it, double *v, int32_t nstate, const int32_t uvwi[3])
{
    if (!it || !v || !uvwi || nstate < 1) return CMDG_ERR_INVALID;
    const InterpObj *o = reinterpret_cast<const InterpObj *>(it);
    std::optional<DevGuard> guard_;
    if (h) guard_.emplace(h->eng);
    std::string err;
    if (h && h->eng->dev != interp_device(o))
        return object_call_done(h, CMDG_ERR_INVALID, "cmdg_interp_project: the object lives on another device than the handle");
    ObjectDevice dev_(interp_device(o));
    return object_call_done(h, interp_project(o, v, nstate, uvwi, h ? h->eng->s_comp : nullptr, !h, err), err);
}

int cmdg_interp_scatter(cmdg_handle h, const cmdg_interp *its, int32_t n, const double *const *v, int32_t nstate,
                        double *fiv)
{
    if (!its || !v || !fiv || n < 1 || nstate < 1) return CMDG_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (!its[i]) return CMDG_ERR_INVALID;
    const InterpObj *const *o = reinterpret_cast<const InterpObj *const *>(its);
    std::optional<DevGuard> guard_;
    if (h) guard_.emplace(h->eng);
    std::string err;
    if (h && h->eng->dev != interp_device(o[0]))
        return object_call_done(h, CMDG_ERR_INVALID, "cmdg_interp_scatter: the objects live on another device than the handle");
    ObjectDevice dev_(interp_device(o[0]));
    return object_call_done(h, interp_scatter(o, n, v, nstate, fiv, h ? h->eng->s_comp : nullptr, !h, err), err);
}

int cmdg_interp_gcm_finish(cmdg_handle h, const cmdg_interp *its, int32_t n, const double *const *vG,
                           const double *const *vB, double *fiv)
{
    if (!its || !vG || !vB || !fiv || n < 1) return CMDG_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (!its[i]) return CMDG_ERR_INVALID;
    const InterpObj *const *o = reinterpret_cast<const InterpObj *const *>(its);
    std::optional<DevGuard> guard_;
    if (h) guard_.emplace(h->eng);
    std::string err;
    if (h && h->eng->dev != interp_device(o[0]))
        return object_call_done(h, CMDG_ERR_INVALID, "cmdg_interp_gcm_finish: the objects live on another device than the handle");
    ObjectDevice dev_(interp_device(o[0]));
    return object_call_done(h, interp_gcm_finish(o, n, vG, vB, fiv, h ? h->eng->s_comp : nullptr, !h, err), err);
}

}  // extern "C"
