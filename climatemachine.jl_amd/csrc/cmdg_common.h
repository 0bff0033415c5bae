// Shared device-side definitions for libcmdg (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cmdg {

// vgeo column ids, 0-based (reference ids Grids.jl:76-92 minus one)
enum { XI1X1 = 0, XI2X1, XI3X1, XI1X2, XI2X2, XI3X2, XI1X3, XI2X3, XI3X3, VM, VMI };
constexpr int JCV = 15;  // _JcV, the vertical line-integral weight the column operators read
// sgeo row ids (Grids.jl:129-130)
enum { SN1 = 0, SN2, SN3, SSM, SVMI };
enum { DIR_EVERY = 0, DIR_HORIZONTAL = 1, DIR_VERTICAL = 2 };
enum {
    NF_RUSANOV = 0, NF_CENTRAL = 1, NF_ROE = 2, NF_HLLC = 3, NF_LMARS = 4,
    // RoeNumericalFluxMoist(LM, HH, LV, LVPP) of the moist AtmosModel (AtmosModel.jl:1276-1513):
    // plain, low-Mach, Harten-Hyman, LeVeque, positivity-preserving LeVeque
    NF_ROE_MOIST = 5, NF_ROE_MOIST_LM = 6, NF_ROE_MOIST_HH = 7, NF_ROE_MOIST_LV = 8,
    NF_ROE_MOIST_LVPP = 9
};
enum { BS_FIRST = 0, BS_GRADIENT = 1 };

constexpr int NXCD = 8;

struct GridDev {
    const double *vgeo, *sgeo;
    const int64_t *vmapM, *vmapP, *elemtobndy;
    const double *D;   // device, (Nq, Nq) column-major, horizontal
    const double *Dv;  // device, (Nqv, Nqv) column-major, vertical (== D for one order)
    int nvgeo;
    // Face tables digested once at cmdg_create from the reference's (sgeo, vmap-, vmap+,
    // elemtobndy), real elements only, indexed by the face task t = 0 .. NFT-1 of an element:
    //   faceP[e][t]     int32, 0-based global node id of the plus side (eP * Np + vidP; the
    //                   minus node itself on boundary faces, DGModel_kernels.jl:686-692)
    //   faceG[e][c][t]  n1, n2, n3, sM (c = 0..3), one coalesced load per component
    //   faceW[e][t]     vMI * sM, the lift weight of the face node: the one product the gradient,
    //                   Laplacian and gradient-of-Laplacian passes need either factor for, so
    //                   they read neither the MI column at the face nodes nor the sM row
    //   facePr[e][t]    faceP with the plus-side node in the ring order below (eP * Np +
    //                   ring_slot(vidP)): what k_gradlap<..., RING> of a hand-off run is handed as
    //                   faceP, so that its gather needs no arithmetic of its own
    // vmap- is a pure function of (f, n) (checked at create) and vMI is MI of that node
    // (Grids.jl:1097-1101, checked at create): neither is stored.  48 B per face node
    // instead of the 56 B of the reference tables; a pass reads 36 of them.
    const int32_t *faceP;
    const double *faceG;
    const double *faceW;
    const int32_t *facePr;
};

// Ghost exchange without pack / unpack launches (handles with neighbours; every pointer is NULL
// otherwise).  The wire format is the reference's (nstate, nvmap) state-fastest buffer of
// kernel_fillsendbuf! / kernel_transferrecvbuf! (MPIStateArrays.jl:837-871).
//   sender:   the exterior launch of a pass copies the element's nodes of vmapsend out of LDS into
//             the send buffer of every array it produces (the nodes of vmapsend all belong to
//             exterior elements, Topologies.jl:250-251);
//   receiver: the plus side of a face whose neighbour is a ghost element is read from the receive
//             buffer of the array instead of from the ghost element.
struct SendEnt {
    int32_t node;  // node of the element, 0-based
    int32_t pos;   // position in vmapsend, 0-based
};
struct HaloDev {
    const int32_t *sendoff;    // (nreal + 1) CSR over the real elements; NULL: this launch sends nothing
    const SendEnt *sendent;    // ascending position within an element
    double *send[2];           // send buffers of this pass's outputs (NULL: not exchanged)
    const int32_t *ghostslot;  // (nghost * Np) position in vmaprecv of a ghost node; NULL: the ghost
                               // elements hold the data (exchanges are unpacked)
    const double *recvQ, *recvGF, *recvHG, *recvHD;
    int64_t nreal;
};

// NQ = horizontal points per direction, NQV = vertical ones (polynomialorder = (N_h, N_v);
// reference: `info.Nq`, `info.Nqk`, `Nfp_h`, `Nfp_v` of basic_grid_info, SpaceDiscretization.jl:18-60)
template <int NQ, int NQV = NQ>
struct KDims {
    static constexpr int Nij = NQ * NQ;
    static constexpr int Np = NQ * NQ * NQV;
    static constexpr int Nfph = NQ * NQV;  // faces 1..4
    static constexpr int Nfpv = NQ * NQ;   // faces 5, 6
    // stride of the face tables: sgeo / vmap are (Nfp_max, nface, nelem) (Metrics.jl:485-488)
    static constexpr int Nfp = Nfph > Nfpv ? Nfph : Nfpv;
    static constexpr int NFT = 4 * Nfph + 2 * Nfpv;  // face-node tasks per element
    static constexpr int NT = (((Np > NFT ? Np : NFT) + 63) / 64) * 64;
    __device__ __forceinline__ static void face_task(int t, int &f, int &n)
    {
        if constexpr (NQ == NQV) {
            f = t / Nfp;
            n = t % Nfp;
        } else if (t < 4 * Nfph) {
            f = t / Nfph;
            n = t % Nfph;
        } else {
            f = 4 + (t - 4 * Nfph) / Nfpv;
            n = (t - 4 * Nfph) % Nfpv;
        }
    }
};

// Face-contiguous ("ring") node order of the Laplacian records of a hand-off run (PassArgs::lapr;
// kernels.h GradArgHandoff).  Slot of node n = (i, j, k): the 4 (NQ - 1)
// perimeter columns (i, j) first, in the order one walks round the square -- along j = 0, up
// i = NQ - 1, back along j = NQ - 1, down i = 0 --, the interior columns after them, the NQV levels
// of a column consecutive.  The NQ * NQV nodes of a lateral face then fill one run of consecutive
// slots (the face i = 0 closes the ring: its run wraps from the last perimeter column to the first),
// so a plus-side gather of node-major records touches the lines of one contiguous piece of the
// neighbour instead of records NQ apart (xi1 faces) or runs of NQ records (xi2 faces).
__host__ __device__ __forceinline__ constexpr int ring_slot_of(int NQ, int NQV, int n)
{
    const int i = n % NQ, j = (n / NQ) % NQ, k = n / (NQ * NQ), E = NQ - 1;
    const int c = j == 0 ? i
                  : i == E ? E + j
                  : j == E ? 2 * E + (E - i)
                  : i == 0 ? 3 * E + (E - j)
                           : 4 * E + (i - 1) + (NQ - 2) * (j - 1);
    return c * NQV + k;
}
// ... and the node that sits in a slot
__host__ __device__ __forceinline__ constexpr int ring_node_of(int NQ, int NQV, int slot)
{
    const int c = slot / NQV, k = slot - c * NQV, E = NQ - 1, NI = NQ > 2 ? NQ - 2 : 1;
    const int q = c - 4 * E;
    const int i = c <= E ? c : c <= 2 * E ? E : c <= 3 * E ? 3 * E - c : c < 4 * E ? 0 : 1 + q % NI;
    const int j = c <= E ? 0 : c <= 2 * E ? c - E : c <= 3 * E ? E : c < 4 * E ? 4 * E - c : 1 + q / NI;
    return i + NQ * (j + NQ * k);
}
template <int NQ, int NQV = NQ>
__host__ __device__ __forceinline__ constexpr int ring_slot(int n)
{
    return ring_slot_of(NQ, NQV, n);
}
template <int NQ, int NQV = NQ>
__host__ __device__ __forceinline__ constexpr int ring_node(int slot)
{
    return ring_node_of(NQ, NQV, slot);
}
// what every build proves of the map: it is a bijection of the element's nodes, and the nodes of
// each lateral face (faces 0..3: i = 0, i = NQ - 1, j = 0, j = NQ - 1) are one cyclic run of the
// perimeter's slots
template <int NQ, int NQV>
constexpr bool ring_order_ok()
{
    constexpr int Np = NQ * NQ * NQV, R = 4 * (NQ - 1) * NQV, Nfph = NQ * NQV;
    for (int n = 0; n < Np; ++n) {
        const int s = ring_slot<NQ, NQV>(n);
        if (s < 0 || s >= Np || ring_node<NQ, NQV>(s) != n) return false;
    }
    for (int s = 0; s < Np; ++s)
        if (ring_slot<NQ, NQV>(ring_node<NQ, NQV>(s)) != s) return false;
    for (int f = 0; f < 4; ++f) {
        bool on[R] = {};
        int count = 0;
        for (int n = 0; n < Np; ++n) {
            const int i = n % NQ, j = (n / NQ) % NQ;
            if (f == 0 ? i == 0 : f == 1 ? i == NQ - 1 : f == 2 ? j == 0 : j == NQ - 1) {
                const int s = ring_slot<NQ, NQV>(n);
                if (s >= R || on[s]) return false;
                on[s] = true;
                ++count;
            }
        }
        if (count != Nfph) return false;
        int starts = 0;  // slots of the face whose cyclic predecessor is not of the face: one per run
        for (int s = 0; s < R; ++s)
            if (on[s] && !on[(s + R - 1) % R]) ++starts;
        if (starts != 1) return false;
    }
    return true;
}
// the orders the library instantiates with a hand-off (DryAtmos with hyperdiffusion, one element
// per work-group: N = 2..4), and the neighbouring ones
static_assert(ring_order_ok<3, 3>() && ring_order_ok<4, 4>() && ring_order_ok<5, 5>(), "ring order");
static_assert(ring_order_ok<2, 2>() && ring_order_ok<6, 6>() && ring_order_ok<7, 7>(), "ring order");
static_assert(ring_order_ok<5, 3>() && ring_order_ok<3, 5>() && ring_order_ok<5, 2>(), "ring order");

// Blocks b and b+8 share an XCD (and its L2); hand each XCD a contiguous run of the
// element list so face neighbours (adjacent in the stacked/Hilbert order) hit one L2.
__device__ __forceinline__ int64_t xcd_remap(int64_t b, int64_t G)
{
    const int64_t q = G / NXCD, r = G % NXCD;
    const int64_t x = b % NXCD, y = b / NXCD;
    return x * q + (x < r ? x : r) + y;
}

template <int N>
__device__ __forceinline__ void fill_negzero(double (&a)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) a[i] = -0.0;
}
// zero-length-safe local array (C++ forbids T[0])
template <int N>
struct Vec {
    double v[N > 0 ? N : 1];
    __device__ __forceinline__ double &operator[](int i) { return v[i]; }
    __device__ __forceinline__ const double &operator[](int i) const { return v[i]; }
    __device__ __forceinline__ operator double *() { return v; }
    __device__ __forceinline__ operator const double *() const { return v; }
    __device__ __forceinline__ void negzero()
    {
#pragma unroll
        for (int i = 0; i < (N > 0 ? N : 1); ++i) v[i] = -0.0;
    }
};

template <int NVAR, int Np>
__device__ __forceinline__ void load_state(Vec<NVAR> &dst, const double *__restrict__ arr, int ijk,
                                           int64_t e)
{
#pragma unroll
    for (int s = 0; s < NVAR; ++s) dst[s] = arr[ijk + (int64_t)Np * (s + (int64_t)NVAR * e)];
}

// position in vmaprecv of the plus-side node (eP, vidP), -1 when it is read from its element
template <int Np>
__device__ __forceinline__ int ghost_slot(const HaloDev &h, int64_t eP, int vidP)
{
    return (h.ghostslot != nullptr && eP >= h.nreal) ? h.ghostslot[(eP - h.nreal) * Np + vidP] : -1;
}
// the first NLOAD of the NVAR columns of the plus-side node: from its element, or from the
// receive buffer of the array (gslot >= 0), whose positions hold NVR columns
template <int NVAR, int Np, int NLOAD, int NVR = NVAR>
__device__ __forceinline__ void load_plus(Vec<NLOAD> &dst, const double *__restrict__ arr,
                                          const double *__restrict__ recv, int gslot, int vidP,
                                          int64_t eP)
{
    if (gslot >= 0) {
#pragma unroll
        for (int s = 0; s < NLOAD; ++s) dst[s] = recv[s + (int64_t)NVR * gslot];
    } else {
#pragma unroll
        for (int s = 0; s < NLOAD; ++s) dst[s] = arr[vidP + (int64_t)Np * (s + (int64_t)NVAR * eP)];
    }
}
// Qhypervisc_grad inside the library (round 4): node-major within an element, (NHG, Np, nelem)
// instead of the reference's (Np, NHG, nelem).  A plus-side gather of a face node then reads NHG * 8
// contiguous bytes instead of NHG values at a stride of Np * 8: on a xi1 / xi2 face of an N = 4
// element the column-major form touches every 128-byte line of all NHG columns of the neighbour
// (5 x the bytes used), the node-major form 1.3-2.3 x.  The volume reads are one contiguous
// record per thread, the stores go out of LDS in memory order.  The library owns this array: a
// Qhypervisc_grad handed to cmdg_create is not written by an evaluation, only by
// cmdg_export_hypervisc_grad, which copies the reference layout out.
template <bool NODE_MAJOR, int NCOL, int Np>
__device__ __forceinline__ int64_t col_at(int n, int s, int64_t e)
{
    return NODE_MAJOR ? s + (int64_t)NCOL * (n + (int64_t)Np * e) : n + (int64_t)Np * (s + (int64_t)NCOL * e);
}
template <int NHG, int Np>
__device__ __forceinline__ int64_t hg_at(int n, int s, int64_t e)
{
    return col_at<true, NHG, Np>(n, s, e);
}
template <int NHG, int Np, int NLOAD>
__device__ __forceinline__ void load_plus_hg(Vec<NLOAD> &dst, const double *__restrict__ arr,
                                             const double *__restrict__ recv, int gslot, int vidP, int64_t eP)
{
    if (gslot >= 0) {
#pragma unroll
        for (int s = 0; s < NLOAD; ++s) dst[s] = recv[s + (int64_t)NHG * gslot];
    } else {
#pragma unroll
        for (int s = 0; s < NLOAD; ++s) dst[s] = arr[hg_at<NHG, Np>(vidP, s, eP)];
    }
}
// the first NW of the NHG columns of element e of a node-major array out of LDS (src[s * Np + n])
// in memory order
template <int NHG, int Np, int NW>
__device__ __forceinline__ void store_node_major(double *__restrict__ arr, int64_t e, int tid, int nthreads,
                                                 const double *src)
{
    double *dst = arr + (int64_t)NHG * Np * e;
    for (int m = tid; m < NHG * Np; m += nthreads) {
        const int n = m / NHG, s = m - n * NHG;
        if (NW == NHG || s < NW) dst[m] = src[s * Np + n];
    }
}
// all NHG columns of element e out of LDS in memory order, the records in the ring order
template <int NHG, int NQ, int NQV>
__device__ __forceinline__ void store_ring_major(double *__restrict__ arr, int64_t e, int tid, int nthreads,
                                                 const double *src)
{
    constexpr int Np = KDims<NQ, NQV>::Np;
    double *dst = arr + (int64_t)NHG * Np * e;
    for (int m = tid; m < NHG * Np; m += nthreads) {
        const int r = m / NHG, s = m - r * NHG;
        dst[m] = src[s * Np + ring_node<NQ, NQV>(r)];
    }
}
// exterior launches: the element's nodes of vmapsend into send buffer `which` (NVAR columns per
// position, the first NW written); value(s, node) is the value the pass stores for the node
template <int NVAR, int NW, class F>
__device__ __forceinline__ void send_nodes(const HaloDev &h, int which, int64_t e, int tid,
                                           int nthreads, F value)
{
    if (h.sendoff == nullptr || h.send[which] == nullptr) return;
    const int b1 = h.sendoff[e + 1];
    for (int k = h.sendoff[e] + tid; k < b1; k += nthreads) {
        const SendEnt ent = h.sendent[k];
        double *dst = h.send[which] + (int64_t)NVAR * ent.pos;
#pragma unroll
        for (int s = 0; s < NW; ++s) dst[s] = value(s, ent.node);
    }
}

}  // namespace cmdg
