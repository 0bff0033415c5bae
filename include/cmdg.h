/* libcmdg -- MI355X-native DG right-hand side + low-storage Runge-Kutta stepping for
 * ClimateMachine-style balance laws.  C ABI: plain pointers and sizes, no C++ or
 * torch types.  One handle per (rank, GPU); a handle is driven by one host thread.
 *
 * The reference (ClimateMachine.jl, Julia) has no FFI seam on this path: the seam
 * is the Julia callable `(dg::DGModel)(tendency, Q, _, t, alpha, beta)`.  Each
 * entry point below names the reference interface it replaces (paths relative to
 * the reference root).  INTEGRATION.md shows the Julia `ccall` stubs.
 *
 * All arrays use the reference's column-major layouts and 1-based integer tables:
 *   state arrays (Np, nstate, nelem) Float64, nelem = nreal + nghost, real first
 *   vgeo (Np, nvgeo, nelem)   sgeo (5, Nfp, nface, nelem)     [Grids.jl:76-146]
 *   vmapM/vmapP (Nfp, nface, nelem) Int64                     [Grids.jl:559-637]
 *   elemtobndy (nface, nelem) Int64                           [Topologies.jl]
 * "device" pointers must stay valid from cmdg_create to cmdg_destroy.
 * Every function returns 0 (CMDG_OK) or a negative cmdg_status; none throws.
 *
 * Environment (read when a handle is created; none is needed in normal use):
 *   CMDG_RCCL_LIB          path of the RCCL library to use (default: the one already in the process,
 *                          e.g. torch's, else librccl.so.1)
 *   CMDG_ROCTX=1           load the roctx library so that the phases of an evaluation carry ranges
 *                          (cmdg:halo:pack / transport / end, cmdg:<pass>[:exterior]); they are
 *                          emitted anyway when rocprofv3 --marker-trace has loaded it
 *   CMDG_REFERENCE_HALO=1, CMDG_HALO_PIPELINE=0   initial values of the two exchange options below
 *   CMDG_HALO_PRIORITY=1   create the halo stream with the highest stream priority
 */
#ifndef CMDG_H
#define CMDG_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cmdg_context *cmdg_handle;

typedef enum cmdg_status {
    CMDG_OK = 0,
    CMDG_ERR_INVALID = -1,     /* bad argument / unsupported configuration */
    CMDG_ERR_HIP = -2,         /* a HIP runtime call failed */
    CMDG_ERR_NO_DEVICE = -3,   /* no gfx950 device visible */
    CMDG_ERR_COMM = -4,        /* RCCL / transport failure */
    CMDG_ERR_UNSUPPORTED = -5  /* physics / polynomial order not compiled in */
} cmdg_status;

/* directions (src/Numerics/Mesh/Grids.jl Direction types) */
enum { CMDG_EVERY_DIRECTION = 0, CMDG_HORIZONTAL_DIRECTION = 1, CMDG_VERTICAL_DIRECTION = 2 };
/* first-order numerical flux (NumericalFluxes.jl:219,298); second order and gradient
 * fluxes are the central ones (:668, :65), as in every configuration in scope */
enum {
    CMDG_RUSANOV = 0, CMDG_CENTRAL_FIRST_ORDER = 1,
    /* methods the dry AtmosModel defines for itself (src/Atmos/Model/AtmosModel.jl:1006,
     * :1154, :1515); CMDG_PHYSICS_DRY_ATMOS without orientation / reference state only */
    CMDG_ROE = 2, CMDG_HLLC = 3, CMDG_LMARS = 4,
    /* RoeNumericalFluxMoist(; LM, HH, LV, LVPP) of the moist AtmosModel (AtmosModel.jl:1276-1513):
     * CMDG_PHYSICS_MOIST_ATMOS with constant viscosity, N = 4 */
    CMDG_ROE_MOIST = 5, CMDG_ROE_MOIST_LM = 6, CMDG_ROE_MOIST_HH = 7, CMDG_ROE_MOIST_LV = 8,
    CMDG_ROE_MOIST_LVPP = 9
};
/* balance laws carried as device functors (pointwise Julia physics cannot cross a C ABI) */
enum {
    CMDG_PHYSICS_ADVECTION_DIFFUSION = 1, CMDG_PHYSICS_DRY_ATMOS = 2,
    CMDG_PHYSICS_HYDROSTATIC_BOUSSINESQ = 3,
    CMDG_PHYSICS_PRESSURE_GRADIENT = 4, /* PressureGradientModel, ref_state.jl:196-233 */
    CMDG_PHYSICS_SHALLOW_WATER = 5,     /* ShallowWaterModel (barotropic half of the split-explicit
                                           ocean), on a one-layer extrusion of the 2-D grid */
    CMDG_PHYSICS_MOIST_ATMOS = 6,       /* AtmosModel LES configuration with EquilMoist
                                           (src/Atmos/Model/moisture.jl:70-115) */
    /* the older split-explicit ocean, src/Ocean/SplitExplicit01: OceanModel, the
     * Continuity3dModel its update_auxiliary_state! evaluates, and the BarotropicModel (on the
     * one-layer extrusion of the 2-D grid) */
    CMDG_PHYSICS_OCEAN_SE01 = 7, CMDG_PHYSICS_CONTINUITY3D_SE01 = 8,
    CMDG_PHYSICS_BAROTROPIC_SE01 = 9,
    /* AtmosAcousticGravityLinearModel of the dry AtmosModel (src/Atmos/Model/linear.jl), on the
     * full model's parameter block and auxiliary array (orientation + reference state) */
    CMDG_PHYSICS_ATMOS_LINEAR_AG = 10,
    /* AtmosAcousticGravityLinearModel of the moist AtmosModel (EquilMoist, linear.jl:57-72): six
     * states, on the full CMDG_PHYSICS_MOIST_ATMOS model's parameter block and 19-column
     * auxiliary array; N = 4, 6; Rusanov or central first-order flux */
    CMDG_PHYSICS_MOIST_LINEAR_AG = 11,
    /* DryAtmosModel of the entropy-stable discretisation (test/Numerics/ESDGMethods/DryAtmos/
     * DryAtmos.jl, total_energy = false, fluctuation_gravity = false): cmdg_create_esdg only */
    CMDG_PHYSICS_ESDG_DRY_ATMOS = 12,
    /* AtmosAcousticLinearModel (linear.jl:214-245) of a dry AtmosModel with NoOrientation() and a
     * reference state: no gravity source, e_pot = 0; on the full model's parameter block and
     * 12-column auxiliary array; N = 4; Rusanov or central first-order flux */
    CMDG_PHYSICS_ATMOS_LINEAR_ACOUSTIC = 13,
    /* DryAtmosAcousticGravityLinearModel (test/Numerics/ESDGMethods/DryAtmos/linear.jl) of the
     * CMDG_PHYSICS_ESDG_DRY_ATMOS model with a reference state: an ordinary DGModel law (cmdg_create)
     * on that model's parameter block and 8-column auxiliary array; N = 3, 4; Rusanov or central
     * first-order flux */
    CMDG_PHYSICS_ESDG_DRY_ATMOS_LINEAR_AG = 14,
    /* VorticityModel (src/Diagnostics/vorticity_balancelaw.jl): state Omega_bl (3), auxiliary u (3)
     * filled by the caller, first-order flux the antisymmetric matrix of u, every boundary tag the
     * `nothing` condition; with CMDG_CENTRAL_FIRST_ORDER and beta = 0 the tendency is curl u in weak
     * form.  N = 2..6, one order in every direction */
    CMDG_PHYSICS_VORTICITY = 15
};

/* Construction record: the fields of `DGModel(balance_law, grid, nf1, nf2, nfgrad;
 * state_auxiliary, state_gradient_flux, states_higher_order, direction,
 * diffusion_direction)` (src/Numerics/DGMethods/DGModel.jl:22-65) and of the
 * `DiscontinuousSpectralElementGrid` it reads (src/Numerics/Mesh/Grids.jl:187-264). */
typedef struct cmdg_desc {
    int32_t dim;                 /* 3 */
    int32_t N[3];                /* polynomial orders (horizontal, horizontal, vertical);
                                    N[0] == N[1]; N[2] may differ (polynomialorder = (N_h, N_v),
                                    Grids.jl:187-264) for the combinations compiled in */
    int64_t nreal, nghost;       /* topology.realelems / ghostelems counts */
    int32_t nvgeo;               /* columns of vgeo (25: GeometricFactors.jl:60-67) */
    int32_t physics_id;          /* CMDG_PHYSICS_* */
    int32_t iparam[16];          /* law parameters, see csrc/physics_*.h */
    double dparam[64];
    int32_t nf_first;            /* CMDG_RUSANOV | CMDG_CENTRAL_FIRST_ORDER | CMDG_ROE | CMDG_HLLC | CMDG_LMARS */
    int32_t direction;           /* dg.direction */
    int32_t diffusion_direction; /* dg.diffusion_direction */
    int32_t stacked;             /* isstacked(grid.topology): with a vertical-only
                                    direction no halo is exchanged (DGModel.jl:104-108) */
    /* grid tables, device pointers */
    const double *vgeo, *sgeo;
    const int64_t *vmapM, *vmapP, *elemtobndy;
    const int64_t *interiorelems;
    int64_t ninterior;           /* grid.interiorelems (1-based) */
    const int64_t *exteriorelems;
    int64_t nexterior;           /* grid.exteriorelems (1-based) */
    const uint8_t *activedofs;   /* (Np*nelem) grid.activedofs, may be NULL if unused */
    const double *D;             /* HOST pointer, (Nq, Nq) column-major, grid.D[1] */
    /* halo tables: grid.vmapsend / vmaprecv (device) and per-neighbour ranges (host) */
    const int64_t *vmapsend;
    int64_t nvmapsend;
    const int64_t *vmaprecv;
    int64_t nvmaprecv;
    int32_t nnabr;
    const int32_t *nabrtorank;       /* HOST, nnabr */
    const int64_t *nabrtovmapsend;   /* HOST, 2*nnabr: first,last (1-based inclusive) */
    const int64_t *nabrtovmaprecv;   /* HOST, 2*nnabr */
    /* arrays owned by the `dg` in the reference; device pointers, caller-owned.
     * state_auxiliary is required; the other three may be NULL (library allocates). */
    double *state_auxiliary;       /* (Np, naux, nelem) */
    double *state_gradient_flux;   /* (Np, ngradflux, nelem); physics_id 2: filled by
                                      cmdg_export_gradient_flux only (see there) */
    double *Qhypervisc_grad;       /* (Np, 3*ngradlap, nelem)  create_states.jl:22-26; filled by
                                      cmdg_export_hypervisc_grad only (see there) */
    double *Qhypervisc_div;        /* (Np, nhyper, nelem) */
    const double *Dv;              /* HOST pointer, (Nqv, Nqv) column-major, grid.D[end]; may be
                                      NULL when N[2] == N[0] */
} cmdg_desc;

/* ---- queries ------------------------------------------------------------------ */
const char *cmdg_version(void);
const char *cmdg_status_string(int status);
/* number_states(balance_law, st) for st = Prognostic, Auxiliary, Gradient, GradientFlux,
 * GradientLaplacian, Hyperdiffusive (src/BalanceLaws/state_types.jl:40-108) -> out[6] */
int cmdg_physics_counts(int32_t physics_id, const int32_t *iparam, int32_t out[6]);
/* CMDG_PHYSICS_DRY_ATMOS: the constants the library derives on the host from the parameter block
 * and hands to its kernels (no device needed) -> out[7]: 1 / (40 day), 1 / day, 1 / (4 day),
 * R_d / cp_d, cp_d / cv_d, (cp_d / cv_d) R_d, R_d / R_d */
int cmdg_atmos_host_constants(const int32_t *iparam, const double *dparam, double out[7]);

/* ---- probes, for the tests only (no handle, no grid) ------------------------------ */
/* q_quot[i]: a[i] over b[i] by the shared-reciprocal quotient the balance laws use (csrc/exact_quotient.h,
 * the pair made from b[i] on the device); q_div[i] = a[i] / b[i].  DEVICE pointers, n doubles each. */
int cmdg_probe_quot(const double *a, const double *b, double *q_quot, double *q_div, int64_t n);
/* CMDG_PHYSICS_DRY_ATMOS with orientation, reference state and DryBiharmonic (the Held-Suarez
 * instantiation; anything else CMDG_ERR_UNSUPPORTED): its pointwise functions at npts points, row-major
 * Q (npts, 5), aux (npts, 17), nrm (npts, 3), der (npts, 2: sin and cos of the latitude) ->
 * out (npts, 33): flux_first_order[15], wavespeed[5], source[5], gradient_argument[8].
 * where = 1: DEVICE pointers, one thread per point; where = 0: HOST pointers, the same text on the host. */
int cmdg_probe_dry_atmos_pointwise(const int32_t *iparam, const double *dparam, int32_t where, const double *Q,
                                   const double *aux, const double *nrm, const double *der, double *out,
                                   int64_t npts);

/* ---- lifetime ----------------------------------------------------------------- */
/* replaces DGModel(...) construction, DGModel.jl:22-65.
 * Preconditions on the grid tables, checked on the device at create (CMDG_ERR_INVALID with the
 * message in cmdg_last_error(NULL) otherwise) -- every grid DiscontinuousSpectralElementGrid
 * builds satisfies them:
 *   - vmapM is the canonical face numbering of Grids.jl:586-594 (vmapM[n, f, e] = the volume node
 *     of face node n of face f of element e): the kernels compute it instead of loading it;
 *   - sgeo's vMI equals vgeo's MI at the face node, bit for bit (Grids.jl:1097-1101);
 *   - plus-side node ids fit 32 bits (nelem * Np < 2^31).
 * The handle keeps a digest of the face tables of its own next to the caller's arrays: 36 B per
 * face node of the real elements (int32 plus-side node + normal + sM); handles with neighbours
 * add 8 B per node of vmapsend and 4 B per ghost node. */
int cmdg_create(const cmdg_desc *desc, cmdg_handle *out);
int cmdg_destroy(cmdg_handle h);

/* Finite-volume reconstruction of a DGFVModel: FVConstant / FVLinear{W}(limiter)
 * (src/Numerics/DGMethods/FVReconstructions.jl:60-192). */
enum { CMDG_FV_CONSTANT = 0, CMDG_FV_LINEAR = 1 };
enum { CMDG_FV_VANLEER = 0, CMDG_FV_NOLIMITER = 1 };
/* HBFVReconstruction(atmos, reconstruction) (src/Atmos/Model/reconstructions.jl:15-73): OR-ed into
 * cmdg_fv_desc.reconstruction, wraps either reconstruction; the law must name a pressure primitive. */
enum { CMDG_FV_HYDROSTATIC = 0x100 };
typedef struct cmdg_fv_desc {
    int32_t reconstruction; /* CMDG_FV_CONSTANT | CMDG_FV_LINEAR, optionally | CMDG_FV_HYDROSTATIC */
    int32_t width;          /* width(reconstruction): 0 for the constant, 1..3 for the linear one */
    int32_t limiter;        /* CMDG_FV_VANLEER | CMDG_FV_NOLIMITER */
    int32_t nvertelem;      /* grid.topology.stacksize */
    int32_t periodicstack;  /* grid.topology.periodicstack */
} cmdg_fv_desc;
/* replaces DGFVModel(balance_law, grid, fv_reconstruction, nf1, nf2, nfgrad; direction)
 * construction, src/Numerics/DGMethods/DGFVModel.jl:22-69: spectral-element DG in the horizontal, a
 * cell-centred finite volume method in the vertical, on a grid with polynomialorder = (N_h, 0)
 * (desc->N[2] == 0, desc->Dv may be NULL).  The handle serves cmdg_rhs, cmdg_lsrk_step / _run /
 * _update, the reductions, the halo and the group calls like any other; its evaluations follow
 * (dgfvm::DGFVModel)(tendency, Q, _, t, alpha, beta), DGFVModel.jl:85-320.
 * Refused with CMDG_ERR_INVALID and a message in cmdg_last_error(NULL): N[2] != 0 (and N[2] == 0
 * through cmdg_create), an unstacked grid, nvertelem < 2, width outside 0..3 or 0 with a linear
 * reconstruction, element lists that are not whole stacks, CMDG_FV_HYDROSTATIC on a law without a
 * pressure primitive (AdvectionDiffusion).  CMDG_ERR_UNSUPPORTED: a law or order not compiled in, a
 * law with hyperdiffusive states (DGFVModel.jl:91), a stack too tall for the LDS staging.  Compiled
 * in: AdvectionDiffusion, advection or advection + diffusion, N_h = 1 and 4; the dry atmosphere law
 * at N_h = 4 with constant viscosity and no hyperdiffusion, either without orientation and
 * reference state or with both, with the Rusanov, central, Roe, HLLC or LMARS first-order flux.
 * A stack is staged in 8 Nq^2 (ns nvertelem + ns (nvertelem + 1) + nvertelem) bytes of LDS: up to
 * 64 KiB launches as it is, up to the 160 KiB a work-group may own on gfx950 the handle raises the
 * kernel's dynamic-LDS limit when it is created (74 cells at N_h = 4 with 5 states), beyond that
 * the handle is refused.  On such a
 * handle element filters, cmdg_courant, cmdg_min_node_distance and cmdg_columnlu_create are refused
 * with CMDG_ERR_UNSUPPORTED. */
int cmdg_create_dgfv(const cmdg_desc *desc, const cmdg_fv_desc *fv, cmdg_handle *out);

/* Two-point fluxes of an ESDGModel (DryAtmos.jl:411-539, :564-745; NumericalFluxes.jl:540-581).
 * Volume: NONE, ENTROPY_CONSERVATIVE, CENTRAL, KG.  Surface: NONE, ENTROPY_CONSERVATIVE, RUSANOV,
 * ENTROPY_CONSERVATIVE_PENALTY, MATRIX. */
enum {
    CMDG_ESDG_FLUX_NONE = 0, CMDG_ESDG_FLUX_ENTROPY_CONSERVATIVE = 1, CMDG_ESDG_FLUX_CENTRAL = 2,
    CMDG_ESDG_FLUX_KG = 3, CMDG_ESDG_FLUX_RUSANOV = 4, CMDG_ESDG_FLUX_ENTROPY_CONSERVATIVE_PENALTY = 5,
    CMDG_ESDG_FLUX_MATRIX = 6
};
typedef struct cmdg_esdg_desc {
    int32_t volume_flux;  /* CMDG_ESDG_FLUX_* */
    int32_t surface_flux; /* CMDG_ESDG_FLUX_* */
    double Mcut;          /* MatrixFlux(Mcut, low_mach, kinetic_energy_preserving) */
    int32_t low_mach;
    int32_t kinetic_energy_preserving;
} cmdg_esdg_desc;
/* replaces ESDGModel(balance_law, grid; state_auxiliary, volume_numerical_flux_first_order,
 * surface_numerical_flux_first_order) construction, src/Numerics/DGMethods/ESDGModel.jl:75-94:
 * entropy-stable flux-differencing DG.  The handle serves cmdg_rhs, cmdg_lsrk_step / _run / _update,
 * cmdg_ssprk_step, cmdg_ls3n_step, the reductions, the halo and the group calls like any other;
 * its evaluations follow (esdg::ESDGModel)(tendency, Q, _, t, alpha, beta), ESDGModel.jl:110-316:
 * one exchange of Q, no gradient passes.  desc->nf_first, direction and diffusion_direction are
 * not read; CMDG_OPT_STEP_GRAPH is accepted and has no effect (the handle stays eager), exchanges
 * are always unpacked (CMDG_OPT_REFERENCE_HALO).
 * Refused with a message in cmdg_last_error(NULL) -- CMDG_ERR_UNSUPPORTED: a law other than
 * CMDG_PHYSICS_ESDG_DRY_ATMOS, an order outside {3, 4} or mixed orders, dim == 2;
 * CMDG_ERR_INVALID: an unknown flux id (and cmdg_create with this physics id).  On such a handle
 * element filters, cmdg_set_rhs_hooks, the stack integrals and cmdg_columnlu_create are refused
 * with CMDG_ERR_UNSUPPORTED. */
int cmdg_create_esdg(const cmdg_desc *desc, const cmdg_esdg_desc *esdg, cmdg_handle *out);
/* state_to_entropy_variables! and state_to_entropy (DryAtmos.jl:339-363, :401-409) of every node of
 * the real elements of Q, on the handle's compute stream (follow with cmdg_synchronize, or with a
 * reduction of the same handle): beta (Np, 6, nelem) and eta (Np, 1, nelem) device arrays, either
 * may be NULL; ghost elements are not written.  CMDG_ERR_UNSUPPORTED on a handle that is not an
 * ESDGModel's. */
int cmdg_esdg_entropy(cmdg_handle h, const double *Q, double *beta, double *eta);

/* Balance laws / template combinations outside the compiled set.  In the reference a law's
 * pointwise functions are compiled into the kernels when the model first runs
 * (src/BalanceLaws/interface.jl:37-464, KernelAbstractions); behind a C ABI the equivalent is a
 * plug-in: a shared object built from this library's own kernel headers (csrc/engine.h + a
 * physics_*.h device functor, one translation unit instantiating make_engine<Law, Nq>) that exports
 *   cmdg::EngineBase *cmdg_plugin_make_engine(const cmdg_desc *, char *err, int errlen)
 * and returns NULL for descriptors it does not serve, and
 *   unsigned long cmdg_plugin_abi(void)        -- engine_abi_stamp() of the headers it was built with;
 * a plug-in built against other headers than this library is refused at load.  cmdg_create asks the loaded plug-ins when no
 * compiled-in engine takes a descriptor (a law the library knows in a combination or at an order
 * it was not built for, or a physics_id of the plug-in's own).  cmdg_load_plugin loads one
 * (idempotent; CMDG_ERR_INVALID with the reason in cmdg_last_error(NULL)); the environment variable
 * CMDG_PLUGINS (colon-separated paths) is read at the first create that needs it.
 * climatemachine.jl_amd/plugins.py writes and builds plug-ins with hipcc. */
int cmdg_load_plugin(const char *path);
/* message of the last failure on this handle (never NULL) */
const char *cmdg_last_error(cmdg_handle h);

/* ---- the hot path ------------------------------------------------------------- */
/* replaces (dg::DGModel)(tendency, Q, _, t, alpha, beta), DGModel.jl:85-427:
 *   tendency .= alpha * dQdt(Q, t) + beta * tendency   on real elements;
 * ghost face nodes of Q are refreshed as a side effect; returns when all device work is
 * complete (DGModel.jl:426). */
int cmdg_rhs(cmdg_handle h, double *tendency, double *Q, double t, double alpha, double beta);
/* same, enqueued on the handle's stream without the final wait */
int cmdg_rhs_async(cmdg_handle h, double *tendency, double *Q, double t, double alpha,
                   double beta);
/* replaces dostep!(Q, lsrk::LowStorageRungeKutta2N, p, time) with its update! kernel,
 * LowStorageRungeKuttaMethod.jl:102-158: for s in 1:nstages
 *   dQ = rhs(Q, t + rkc[s] dt) + dQ;  Q += rkb[s] dt dQ;  dQ *= rka[s % nstages + 1]
 * (the update is fused into the last kernel of each stage).  Asynchronous: call
 * cmdg_synchronize before reading Q on another stream or on the host. */
int cmdg_lsrk_step(cmdg_handle h, double *Q, double *dQ, double t, double dt, int32_t nstages,
                   const double *rka, const double *rkb, const double *rkc);
/* nsteps back-to-back steps of size dt starting at t (solve! loop body,
 * ODESolvers.jl:110-158 without callbacks); step i starts at the running sum t + dt + ... + dt,
 * as updatetime! accumulates it (ODESolvers.jl:96-98) */
int cmdg_lsrk_run(cmdg_handle h, double *Q, double *dQ, double t, double dt, int64_t nsteps,
                  int32_t nstages, const double *rka, const double *rkb, const double *rkc);
int cmdg_synchronize(cmdg_handle h);

/* Options of a handle.
 * CMDG_OPT_KEEP_GRADFLUX (default 0): a law whose second-order flux does not read the
 *   gradient-flux state (the dry atmosphere with zero viscosity: tau = -2 nu S = 0) has the
 *   nine columns of dg.state_gradient_flux neither formed, stored nor exchanged -- the tendency
 *   is bit-identical without them.  1 restores the reference's behaviour of refreshing
 *   state_gradient_flux in every evaluation (DGModel.jl:126-206), for callers that read it
 *   (diagnostics, the diffusive Courant number).
 * CMDG_OPT_STACK_HEIGHT (default 0 = unknown): number of elements of a vertical stack of a stacked
 *   topology (length(topology.stacksize); elements of a stack are contiguous, e = ev + (eh - 1) nv).
 *   Results do not depend on it.  With tall stacks (more than 16 elements) the engine walks its
 *   element lists in tiles of 32 columns x 4 levels instead of column by column, so that the
 *   elements in flight on one XCD are horizontal neighbours whose face gathers meet in its L2.
 * CMDG_OPT_REFERENCE_HALO (default 0): handles with neighbours.  By default an evaluation launches
 *   no pack or unpack kernel: the exterior launch of every pass writes the nodes of vmapsend of
 *   what it produces straight into the send buffer, and -- unless the law's nodal
 *   update_auxiliary_state! or the hooks read the ghost ELEMENTS -- the face kernels read the plus
 *   side of ghost neighbours from the receive buffers, so the ghost elements of Q, of
 *   state_gradient_flux and of the hyperdiffusion arrays are NOT refreshed.  Results are
 *   bit-identical.  1 restores begin/end_ghost_exchange! as the reference runs them
 *   (kernel_fillsendbuf! / kernel_transferrecvbuf! around every exchange, MPIStateArrays.jl:411-483),
 *   for callers that read ghost elements after an evaluation (diagnostics, output, a Courant
 *   number over ghosts).  cmdg_halo_begin/end always do.  cmdg_query(CMDG_Q_DIRECT_RECV) says
 *   which mode an evaluation runs in: it turns itself off when hooks or a nodal
 *   update_auxiliary_state! kernel read ghost elements.  Wire format: the reference's (nstate,
 *   nvmap) state-fastest buffers, with one exception in the default mode -- of Qhypervisc_div's
 *   nhyp columns only the ngl the Laplacian pass writes (and the next pass reads) travel.
 * CMDG_OPT_HALO_PIPELINE (default 1): handles whose exchanges run direct both ways launch the
 *   exterior element list of every pass on the halo stream, between the exchange it waits for
 *   and the exchange it feeds (a chain without event hops), and the interior list on the compute
 *   stream one pass behind or ahead (the passes of a step form two loosely coupled pipelines).
 *   0: the reference's order on one compute stream (interior launch, wait, exterior launch).
 *   Results do not depend on it.
 * CMDG_OPT_STEP_GRAPH (default 0; environment CMDG_STEP_GRAPH=1): cmdg_lsrk_run records one step
 *   into a HIP graph and replays it for every step but the first of a run; the evaluation times
 *   live in device memory and advance as updatetime! does.  Results are bit-identical.
 *   Handles that exchange through RCCL are recorded too when their exchanges run direct and
 *   pipelined (CMDG_Q_HALO_PIPELINE): one hipGraphLaunch then stands for the 40 kernel launches,
 *   100 event operations and 20 RCCL groups of a Held-Suarez step.  What crashed in round 3 is
 *   settled (scripts/probe/rccl_capture_probe.py, one fresh process per hypothesis, both stacks):
 *   on HIP 7.0.2 / RCCL 2.26.6 hipStreamEndCapture segfaults if and only if an ncclSend / ncclRecv
 *   group was recorded on a stream that JOINED the capture through an event -- Global or Relaxed
 *   mode alike; on the origin stream every mode, several operations per group and several groups
 *   per capture are fine; ROCm 7.2 / RCCL 2.27.7 accepts both forms (the probes use a rank as its
 *   own peer: whether the crash needs the self-send cannot be told on one GPU, and does not matter
 *   for the remedy).  The
 *   library therefore begins such a capture on the halo stream (the groups' stream) and forks the
 *   compute stream.  Runs a capture cannot hold stay eager: profiling, filters, hooks, a nodal
 *   update_auxiliary_state! kernel of its own, the local transport, exchanges that are packed.
 * CMDG_OPT_TENDENCY_PAIRS, CMDG_OPT_TENDENCY_FOUR_WAVES: retired; accepted and have no effect.
 * CMDG_OPT_ASYNC_RUN (default 0): cmdg_lsrk_run hands the run to a thread the handle owns and
 *   returns at once (the tableau is copied, Q and dQ must stay valid): the calling thread is not the
 *   one that spends ~1 ms per step of a partitioned run inside hipGraphLaunch or posting RCCL
 *   groups.  Runs execute in order; every other entry point of the handle first waits until that
 *   thread is idle, so the handle is still driven by one thread at a time; a deferred run that
 *   failed is reported by the next cmdg_synchronize.  Same launches in the same order: results
 *   are bit-identical.
 * CMDG_OPT_STREAM_PRIORITY (default 0): 1 puts both streams of the handle at the device's highest
 *   stream priority, -1 at the lowest.  Meant for a handle whose launches are small and form a long dependent chain
 *   next to another handle's bandwidth-bound launches (the barotropic model of the split-explicit
 *   ocean, whose sub-steps decide the length of a slow stage).  The handle must be idle; results
 *   do not depend on it.
 * CMDG_OPT_GRADARG_HANDOFF (default 1): inside cmdg_lsrk_run the fused update of a stage also forms
 *   the gradient arguments of the updated state and does the nodal update_auxiliary_state! for
 *   it, and the next stage's gradient pass reads those records instead of Q and state_auxiliary.
 *   Taken only by single-rank handles (no ghost elements) of a law whose gradient-flux state is
 *   not formed, with hyperdiffusion and a fused nodal refresh (Held-Suarez), without hooks,
 *   filters or CMDG_OPT_STEP_GRAPH; the first evaluation and the last update of every run are the
 *   ordinary kernels, so nothing is carried from one call to the next.  Of these updates only the
 *   run's last does the refresh when no pass of the law reads the refreshed columns (the dry
 *   atmosphere's theta_v / air_T): the others would be overwritten unseen.  Q, dQ and every column
 *   of state_auxiliary end a run bit-identical.  cmdg_query(CMDG_Q_GRADARG_HANDOFF) says whether
 *   the last run used it.
 * CMDG_OPT_FUSED_LAPLACIAN (default 1): an evaluation of such a run that reads the records forms the
 *   gradients and their Laplacians in one launch, so that Qhypervisc_grad's intermediate never
 *   goes to memory.  Taken only where the diffusion direction is horizontal and every lateral face
 *   of every real element is interior with a unique opposite face node (decided once at create:
 *   the sphere, laterally periodic bricks more than one element wide); everything else keeps the
 *   two launches.  Bit-identical results.  cmdg_query(CMDG_Q_FUSED_LAPLACIAN) counts the
 *   evaluations of the last run that took it. */
enum {
    CMDG_OPT_KEEP_GRADFLUX = 1, CMDG_OPT_STACK_HEIGHT = 2, CMDG_OPT_REFERENCE_HALO = 3,
    CMDG_OPT_HALO_PIPELINE = 4, CMDG_OPT_STEP_GRAPH = 5, CMDG_OPT_STREAM_PRIORITY = 6,
    CMDG_OPT_TENDENCY_PAIRS = 7 /* retired */, CMDG_OPT_ASYNC_RUN = 8,
    CMDG_OPT_TENDENCY_FOUR_WAVES = 9 /* retired */, CMDG_OPT_GRADARG_HANDOFF = 10,
    CMDG_OPT_FUSED_LAPLACIAN = 11
};
int cmdg_set_option(cmdg_handle h, int32_t option, int32_t value);

/* What the handle's kernels actually do, for byte accounting and tests (no reference counterpart):
 *   GRADFLUX_LIVE         is state_gradient_flux formed by an evaluation (see CMDG_OPT_KEEP_GRADFLUX)
 *   LAW_NEEDS_GRADFLUX    does the tendency pass read it
 *   NDERIVED              columns of handle-owned time-invariant per-node fields the source reads
 *   NUPDATED_AUX          auxiliary columns the law's nodal update_auxiliary_state! rewrites (0: none)
 *   FUSED_UPDATE_AUX      is that refresh fused into the gradient pass
 *   DIRECT_SEND / _RECV   is the ghost exchange running without pack / unpack launches
 *   TENDENCY_ELEMS_PER_GROUP  elements per work-group of the tendency pass
 *   STATE_READ + p, AUX_READ + p   columns of Q / of state_auxiliary the volume code of pass p
 *                         reads (p = 0 gradients, 1 Laplacian, 2 gradient of Laplacian, 3 tendency);
 *                         every column for a law that does not declare less */
enum {
    CMDG_Q_GRADFLUX_LIVE = 1, CMDG_Q_LAW_NEEDS_GRADFLUX = 2, CMDG_Q_NDERIVED = 3,
    CMDG_Q_NUPDATED_AUX = 4, CMDG_Q_FUSED_UPDATE_AUX = 5, CMDG_Q_DIRECT_SEND = 6,
    CMDG_Q_DIRECT_RECV = 7, CMDG_Q_TENDENCY_ELEMS_PER_GROUP = 8,
    CMDG_Q_HALO_PIPELINE = 9, /* are the two pipelines of CMDG_OPT_HALO_PIPELINE in use */
    CMDG_Q_HOST_POST_NS = 10,   /* host nanoseconds spent posting exchanges (RCCL group calls) ... */
    CMDG_Q_HOST_POST_COUNT = 11, /* ... and how many were posted, since the handle was created */
    CMDG_Q_GRAPH_STEPS = 12,     /* steps cmdg_lsrk_run replayed from a captured graph */
    CMDG_Q_TENDENCY_PAIRS = 13,  /* retired with CMDG_OPT_TENDENCY_PAIRS: always -1 (option off) */
    CMDG_Q_GRADARG_HANDOFF = 14, /* did the last cmdg_lsrk_run use CMDG_OPT_GRADARG_HANDOFF */
    CMDG_Q_GRADARG_REFRESHES = 15, /* ... and how many of its hand-off updates carried the nodal auxiliary
                                      refresh: 1 for a law whose refreshed columns no pass reads (only the
                                      last one is ever seen), else all of them; 0 without the hand-off */
    CMDG_Q_STATE_READ = 16, CMDG_Q_AUX_READ = 20,
    CMDG_Q_FUSED_LAPLACIAN = 24 /* evaluations of the last cmdg_lsrk_run that took CMDG_OPT_FUSED_LAPLACIAN:
                                   all but the first (5 K - 1 for K LSRK54 steps) on an eligible handle, else 0 */
};
int cmdg_query(cmdg_handle h, int32_t what, int64_t *out);

/* dg.states_higher_order[1] (Qhypervisc_grad, create_states.jl:22-26) in the reference layout
 * (Np, 3*ngradlap, nelem).  The library keeps its working copy node-major -- (3*ngradlap, Np,
 * nelem): the 3*ngradlap values of a node are contiguous, which is what a plus-side face gather of
 * the Laplacian and tendency passes reads -- so cmdg_desc.Qhypervisc_grad is
 * NOT written by an evaluation; this call writes the array as the reference would hold it after
 * the last evaluation (`dst`, or cmdg_desc.Qhypervisc_grad if dst is NULL) and returns when the
 * copy is complete.  The copy runs on the handle's own (non-blocking) stream: work the caller has
 * pending on `dst` on another stream -- the fill of a freshly allocated array -- must have finished
 * before the call.  Ghost elements as described for CMDG_OPT_REFERENCE_HALO.  For diagnostics
 * and tests: nothing on the hot path reads the reference layout. */
int cmdg_export_hypervisc_grad(cmdg_handle h, double *dst);
/* The same for dg.state_gradient_flux, (Np, ngradflux, nelem).  For the dry atmosphere (physics_id 2)
 * the library's working copy is node-major as well and cmdg_desc.state_gradient_flux is
 * written by this call only; for every other law the array of cmdg_desc IS the working copy (hooks
 * and filters address it) and the call is a no-op (dst NULL or that array) or a copy. */
int cmdg_export_gradient_flux(cmdg_handle h, double *dst);

/* ---- halo (MPIStateArrays.jl:411-514, 837-871) -------------------------------- */
/* begin_ghost_exchange!: pack face nodes of `array` (Np, nstate, nelem) and post the
 * sends/receives; end_ghost_exchange!: wait and unpack into the ghost elements. */
int cmdg_halo_begin(cmdg_handle h, double *array, int32_t nstate);
int cmdg_halo_end(cmdg_handle h, double *array, int32_t nstate);
/* kernel_fillsendbuf! / kernel_transferrecvbuf! (MPIStateArrays.jl:837-871) on their own, for
 * arrays of any (Np, nstate): sendbuf (nstate, nvmap) state-fastest <- buf (Np, nstate, nelem)
 * at the 1-based linear node ids vmapsend[i] = n + Np (e - 1), and the inverse into the ghost
 * elements.  Device pointers; runs on the null stream and returns when done.  (The handle-based
 * exchange above launches the same kernels; these entries let the reference's known-answer
 * test, test/Arrays/mpi_comm.jl:23-153, be replayed on them.) */
int cmdg_fillsendbuf(double *sendbuf, const double *buf, const int64_t *vmapsend, int64_t nvmap,
                     int32_t Np, int32_t nstate);
int cmdg_transferrecvbuf(double *buf, const double *recvbuf, const int64_t *vmaprecv,
                         int64_t nvmap, int32_t Np, int32_t nstate);
/* Transport set-up.  Multi-process: RCCL point-to-point; `unique_id` is the 128-byte
 * ncclUniqueId made by cmdg_comm_unique_id on rank 0 and broadcast by the caller. */
int cmdg_comm_unique_id(void *out128);
int cmdg_comm_init_rccl(cmdg_handle h, const void *unique_id128, int32_t rank, int32_t nranks);
/* Transport self-check: sends `count` doubles to this rank itself with the same
 * ncclGroupStart / ncclRecv / ncclSend / ncclGroupEnd sequence the halo uses, on the halo
 * stream, and verifies the payload.  Needs cmdg_comm_init_rccl first (nranks may be 1). */
int cmdg_comm_selftest(cmdg_handle h, int64_t count);
/* Single-process: connect n handles (handle r plays rank r) through device copies. */
int cmdg_comm_connect_local(cmdg_handle *handles, int32_t n);

/* Entries that take several handles -- cmdg_comm_connect_local, the cmdg_group_* calls,
 * cmdg_group_reduce, the split-explicit steppers (one or n (slow, fast) pairs) and the three
 * cmdg_ocean_* calls (slow, fast) -- refuse a NULL handle list, n < 1 or a NULL handle with
 * CMDG_ERR_INVALID and no message.  Otherwise they first wait for the deferred CMDG_OPT_ASYNC_RUN
 * run of EVERY handle passed.  On failure every handle passed carries the message: the reason,
 * prefixed with the member that failed -- "rank i: " for a list of handles, "pair i (slow): " or
 * "pair i (fast): " for (slow, fast) pairs -- or the bare status string when no member gave one.
 *
 * Lock-step drivers for handles connected with cmdg_comm_connect_local (one host thread
 * plays every rank): arrays of n per-rank pointers. */
int cmdg_group_rhs(cmdg_handle *handles, int32_t n, double **tendency, double **Q, double t,
                   double alpha, double beta);
/* one ghost exchange of a state-like array per handle (begin on all, then end on all):
 * e.g. state_auxiliary columns after initialisation (SpaceDiscretization.jl create_state +
 * MPIStateArrays.begin/end_ghost_exchange!) */
int cmdg_group_halo(cmdg_handle *handles, int32_t n, double **arrays, int32_t nstate);
int cmdg_group_lsrk_run(cmdg_handle *handles, int32_t n, double **Q, double **dQ, double t,
                        double dt, int64_t nsteps, int32_t nstages, const double *rka,
                        const double *rkb, const double *rkc);

/* ---- reductions (MPIStateArrays.jl:583-644), local part; caller all-reduces ---- */
/* out = sum over real elements of M .* A.^2  (weighted) or A.^2 */
int cmdg_norm2_local(cmdg_handle h, const double *A, int32_t nstate, int32_t weighted,
                     double *out_host);
/* out = sum over real elements of M .* (A - B).^2 */
int cmdg_distance2_local(cmdg_handle h, const double *A, const double *B, int32_t nstate,
                         double *out_host);

/* ---- reductions of state arrays, all-reduced (MPIStateArrays.jl:583-807) ------------------
 * weightedsum (:655-674), dot (:608-626), norm for p = 1, 2, any finite p > 0 and INFINITY with
 * or without dims = (1, 3) (:583-604, :676-768), euclidean_distance (:628-644) and sum / maximum /
 * minimum (mapreduce, :775-807) over the real elements of an (Np, nstate, nelem) array; ghost
 * elements are never read.  Sums accumulate in double-double (an unevaluated pair hi + lo, as the
 * reference's DoubleFloat): error-free products (fma) and sums form every term, per thread, wave
 * and block; M (vgeo column VM, the reference's `weights`) times A is exact for _WEIGHTEDSUM.  Per-
 * block partials are folded in a fixed order on the device, with no atomics: the same input gives
 * the same bits on every call.  A NaN in a real element propagates (max / min / inf-norm too).
 * The kernels run on the handle's compute stream after any deferred CMDG_OPT_ASYNC_RUN run. */
enum {
    CMDG_RED_WEIGHTEDSUM = 0, /* sum of M .* A[:, states, :]  (always weighted) */
    CMDG_RED_SUM = 1,         /* sum of A                     (never weighted) */
    CMDG_RED_DOT = 2,         /* sum of (M .*) A .* B */
    CMDG_RED_DISTANCE = 3,    /* sqrt(sum of M .* (A - B).^2) (always weighted) */
    CMDG_RED_NORM = 4,        /* (sum of (M .*) |A|.^p)^(1/p); p = INFINITY: maximum |A|, unweighted */
    CMDG_RED_MAX = 5,         /* maximum of A */
    CMDG_RED_MIN = 6          /* minimum of A */
};
typedef struct cmdg_reduce_desc {
    int32_t op;            /* CMDG_RED_* */
    double p;              /* _NORM only: 1, 2, any finite p > 0, or INFINITY */
    int32_t weighted;      /* _DOT, _NORM (ignored for p = INFINITY); _WEIGHTEDSUM, _DISTANCE always weighted */
    int32_t per_state;     /* 0: one value; 1: one value per chosen state (dims = (1,3)) */
    int32_t nstate;        /* columns of A (and B) */
    const int32_t *states; /* 0-based subset, NULL = all */
    int32_t nstates;
} cmdg_reduce_desc;

/* this rank's unrounded partials: nout (hi, lo) pairs, nout = per_state ? number of chosen states
 * : 1; max / min / inf-norm in hi, lo = 0 */
int cmdg_reduce_local(cmdg_handle h, const cmdg_reduce_desc *d, const double *A, const double *B,
                      double *partials_host);
/* host only, needs no GPU: combines nranks x nout partials in rank order (the exact sum of every
 * hi and lo, correctly rounded to double), applies the finishing power (sqrt / ^(1/p)); what every
 * rank runs after an all-gather of the partials.  Errors: cmdg_last_error(NULL). */
int cmdg_reduce_combine(const cmdg_reduce_desc *d, const double *partials, int32_t nranks,
                        double *out);
/* global value on every rank: single rank = local; RCCL handle = ncclAllGather of the partials
 * on the handle's communicator, then cmdg_reduce_combine; a local-transport handle of a group
 * with n > 1 is refused (CMDG_ERR_INVALID: use cmdg_group_reduce) */
int cmdg_reduce(cmdg_handle h, const cmdg_reduce_desc *d, const double *A, const double *B,
                double *out_host);
/* handles connected with cmdg_comm_connect_local: one host thread plays every rank; A[i], B[i]
 * are rank i's arrays (B may be NULL where the op takes none) */
int cmdg_group_reduce(cmdg_handle *handles, int32_t n, const cmdg_reduce_desc *d,
                      const double **A, const double **B, double *out_host);

/* ---- Courant numbers and time-step selection ------------------------------------------ */
/* local_courant functions of src/Atmos/Model/courant.jl:29-83 and, for the ocean model,
 * src/Ocean/HydrostaticBoussinesq/Courant.jl:13-111 (which adds viscous_courant) */
enum {
    CMDG_ADVECTIVE_COURANT = 0, CMDG_NONDIFFUSIVE_COURANT = 1, CMDG_DIFFUSIVE_COURANT = 2,
    CMDG_VISCOUS_COURANT = 3
};
/* courant(local_courant, dg, m, Q, dt, simtime, direction) (SpaceDiscretization.jl:307-365):
 * maximum over this rank's real nodes of the law's local Courant number, with dx the
 * minimum neighbour distance of the node in `direction`; -inf when the rank owns no element.
 * The caller applies MPI.Allreduce(max) (:364).  calculate_dt (DGMethods.jl:79-83) is
 * Courant_number / cmdg_courant(NONDIFFUSIVE, dt = 1).  Blocks until the value is on the host.
 * An ESDGModel handle serves the advective and the nondiffusive kind of its DryAtmosModel
 * (test/Numerics/ESDGMethods/DryAtmos/DryAtmos.jl:747-793) and refuses the others. */
int cmdg_courant(cmdg_handle h, int32_t kind, const double *Q, double dt, double simtime,
                 int32_t direction, double *out_host);
/* min_node_distance(grid, direction) (Grids.jl:455-486): rank-local minimum, +inf for an empty
 * rank; the caller applies MPI.Allreduce(min). */
int cmdg_min_node_distance(cmdg_handle h, int32_t direction, double *out_host);

/* ---- column (stack) integrals ------------------------------------------------------ */
/* indefinite_stack_integral! / reverse_indefinite_stack_integral! (DGModel.jl:445-529, kernels
 * DGModel_kernels.jl:1903-2104) on stacked topologies (elements of a stack contiguous,
 * e = ev + (eh - 1) nvertelem).  The law's integral_load/set_auxiliary_state! hooks are
 * carried as a field combination: integrand_s = scale_s * field_s, where field_s is column
 * src_col[s] (0-based) of the prognostic state (src_is_state[s] != 0) or of the auxiliary
 * array; the upward integral goes to auxiliary column dst_col[s]; the reverse integral reads
 * auxiliary column rsrc_col[s] and writes (value at the top of the stack) - value to rdst_col[s]. */
#define CMDG_STACK_MAXOUT 8
typedef struct cmdg_stack_integral_desc {
    int32_t nout; /* 1..CMDG_STACK_MAXOUT */
    int32_t src_is_state[CMDG_STACK_MAXOUT], src_col[CMDG_STACK_MAXOUT];
    double scale[CMDG_STACK_MAXOUT];
    int32_t dst_col[CMDG_STACK_MAXOUT];
    int32_t rsrc_col[CMDG_STACK_MAXOUT], rdst_col[CMDG_STACK_MAXOUT];
} cmdg_stack_integral_desc;
/* Q (Np, nstate, nelem) may be NULL when no integrand reads the state; aux (Np, naux, nelem) is
 * updated in place on the real elements; Imat = HOST (Nq, Nq) column-major grid.Imat[dim]
 * (Grids.jl:1184-1207).  Enqueued on the compute stream. */
int cmdg_indefinite_stack_integral(cmdg_handle h, const double *Q, int32_t nstate, double *aux,
                                   int32_t naux, int32_t nvertelem, const double *Imat,
                                   const cmdg_stack_integral_desc *d);
int cmdg_reverse_indefinite_stack_integral(cmdg_handle h, double *aux, int32_t naux,
                                           int32_t nvertelem, const cmdg_stack_integral_desc *d);

/* ---- element filters (src/Numerics/Mesh/Filters.jl) ------------------------------ */
typedef struct cmdg_filter_s *cmdg_filter;
/* AbstractFilter: spectral = Exponential / BoydVandeven / Cutoff (Filters.jl:172-307,
 * kernel_apply_filter! :651-794); MassPreservingCutoffFilter (:316-347, kernel :893-1071);
 * TMARFilter (:369, kernel :796-884) */
enum { CMDG_FILTER_SPECTRAL = 0, CMDG_FILTER_MASS_PRESERVING = 1, CMDG_FILTER_TMAR = 2 };
/* AbstractFilterTarget: FilterIndices (Filters.jl:72-100), AtmosFilterPerturbations and
 * AtmosSpecificFilterPerturbations (src/Atmos/Model/filters.jl:4-118, dry model: the
 * state is rho, rho u[3], rho e and the reference state is read from state_auxiliary) */
enum {
    CMDG_TARGET_INDICES = 0, CMDG_TARGET_ATMOS_PERTURBATIONS = 1,
    CMDG_TARGET_ATMOS_SPECIFIC_PERTURBATIONS = 2
};
#define CMDG_MAX_FILTER_STATES 32
typedef struct cmdg_filter_desc {
    int32_t kind;        /* CMDG_FILTER_* */
    int32_t target;      /* CMDG_TARGET_* */
    int32_t direction;   /* CMDG_*_DIRECTION keyword of Filters.apply! (spectral kinds) */
    int32_t nindices;    /* FilterIndices: number of filtered states */
    int32_t indices[CMDG_MAX_FILTER_STATES]; /* 1-based state indices */
    int32_t aux_ref_rho, aux_ref_rhoe; /* atmos targets: 0-based state_auxiliary columns of
                                          ref_state.rho and ref_state.rho e */
    const double *filter_h; /* HOST (Nq, Nq) column-major filter.filter_matrices[1] */
    const double *filter_v; /* HOST (Nq, Nq) column-major filter.filter_matrices[end] */
} cmdg_filter_desc;
/* filter object bound to a handle: the filter struct + target + direction of one
 * `Filters.apply!(Q, target, grid, filter; direction, state_auxiliary)` call site */
int cmdg_filter_create(cmdg_handle h, const cmdg_filter_desc *d, cmdg_filter *out);
int cmdg_filter_destroy(cmdg_handle h, cmdg_filter f);
/* Filters.apply_async! (Filters.jl:440-607): enqueue on the handle's compute stream, real
 * elements only, in place.  Q is a device array (Np, nstate, nelem); atmos targets read the
 * handle's state_auxiliary.  Follow with cmdg_synchronize for Filters.apply! (:408-421). */
int cmdg_filter_apply(cmdg_handle h, cmdg_filter f, double *Q, int32_t nstate);
/* filters the DG operator and the time stepper apply themselves:
 *   gradient_filter  on state_gradient_flux after the gradient pass   (DGModel.jl:185-193)
 *   tendency_filter  on the tendency at the end of the evaluation      (DGModel.jl:417-425)
 *   step_filter      on Q after every completed LSRK step -- the EveryXSimulationSteps(1)
 *                    callback of experiments/AtmosGCM/heldsuarez.jl:261-272
 * NULL clears a slot.  The filters must outlive their use. */
int cmdg_set_filters(cmdg_handle h, cmdg_filter gradient_filter, cmdg_filter tendency_filter,
                     cmdg_filter step_filter);

/* ---- interpolation onto box and latitude-longitude grids (src/Numerics/Mesh/Interpolation.jl) ---
 * InterpolationBrick (:132-376) and InterpolationCubedSphere (:700-1044) are host set-up
 * (climatemachine.jl_amd/mesh/interpolation.py); the descriptor carries what they produce.  The
 * library copies the point tables to the device and computes the barycentric weights of the nodes
 * itself; the coincidence flags and the scaling the reference stores per point (flg, fac) are
 * formed inside the kernel from xi.  Every pointer of the descriptor is a HOST pointer and need
 * not outlive cmdg_interp_create.  Refused at create (CMDG_ERR_INVALID, message in
 * cmdg_last_error(h)): an offset table that does not start at 0, decreases or does not end at
 * npoints; a xi outside [-1 - 1e-10, 1 + 1e-10] (or NaN); an index triple outside the output grid;
 * npoints or n1 n2 n3 beyond 2^31 - 1.  CMDG_ERR_UNSUPPORTED: Nq[0] != Nq[1], or an Nq outside 2..8.
 * With offset, xi1, xi2 and xi3 all NULL the object holds index triples only (Nq, nelem and xi_nodes are
 * not read): it serves cmdg_interp_project and cmdg_interp_scatter -- a root that scatters the gathered
 * index vectors of every rank -- and cmdg_interp_apply refuses it.
 *
 * The cmdg_handle argument of every entry may be NULL.  With a handle the work is ordered on that
 * handle's compute stream, after any deferred CMDG_OPT_ASYNC_RUN run, and the call returns without
 * waiting (follow with cmdg_synchronize), as the filters do; errors go to cmdg_last_error(h).  With
 * NULL the work runs on the default stream of the device the object was created on and the call
 * returns when it is done; errors go to cmdg_last_error(NULL).  The object is not bound to a
 * handle: polynomial orders no engine is compiled for, such as (5, 6), are served with NULL. */
typedef struct cmdg_interp_s *cmdg_interp;
typedef struct cmdg_interp_desc {
    int32_t Nq[3];             /* points per direction of the grid, polynomialorders(grid) .+ 1 */
    int64_t nelem;             /* length(topology.realelems) */
    int64_t npoints;           /* Npl: output points of this rank */
    const double *xi_nodes[3]; /* referencepoints(grid): Nq[d] LGL nodes per direction */
    const int64_t *offset;     /* nelem + 1 prefix sums, 0-based: element e (0-based) owns the
                                  points offset[e] .. offset[e + 1] - 1 */
    const double *xi1, *xi2, *xi3; /* npoints reference coordinates each */
    const int32_t *i1, *i2, *i3;   /* npoints 1-based indices into the output grid: x1i, x2i, x3i
                                      of the brick; longi, lati, radi of the sphere */
    int64_t n1, n2, n3;        /* output grid: (n1g, n2g, n3g) or (n_long, n_lat, n_rad) */
    const double *lat_grd, *long_grd; /* sphere: n2 latitudes and n1 longitudes in degrees; NULL
                                         for a brick (cmdg_interp_project then refuses) */
} cmdg_interp_desc;
int cmdg_interp_create(cmdg_handle h, const cmdg_interp_desc *d, cmdg_interp *out);
/* waits for the handle h (if given) and for the device's default stream, then frees the tables: work
 * that used the object through ANOTHER handle must have been synchronised by the caller, as for the
 * filters.  No device-wide synchronisation. */
int cmdg_interp_destroy(cmdg_handle h, cmdg_interp it);
/* interpolate_local! (:397-570, :1265-1317): Q (Np, nstate, nelemQ) device array with
 * nelemQ >= nelem, v (npoints, nstate) device array;
 *   v[p, s] = sum_k l3_k(xi3) sum_j l2_j(xi2) sum_i l1_i(xi1) Q[i + Nq1 (j + Nq2 k), s, e]
 * with the Lagrange basis l in barycentric form; a xi within 4 eps of a node picks that node. */
int cmdg_interp_apply(cmdg_handle h, cmdg_interp it, const double *Q, int32_t nstate, int64_t nelemQ,
                      double *v);
/* project_cubed_sphere! (:1332-1414): the three 1-based columns uvwi of v (npoints, nstate), Cartesian
 * components, become the components along the unit vectors in longitudinal, latitudinal and radial
 * direction at each point's latitude and longitude.  A column outside 1..nstate or a column
 * named twice is refused (CMDG_ERR_INVALID). */
int cmdg_interp_project(cmdg_handle h, cmdg_interp it, double *v, int32_t nstate, const int32_t uvwi[3]);
/* the device half of accumulate_interpolated_data! (:1453-1561) for the n ranks of one process:
 * fiv[i1, i2, i3, s] = v[r][p, s] through the index triples of its[r], r = 0 .. n - 1 in order; fiv is
 * (n1, n2, n3, nstate) column-major and the objects must agree on (n1, n2, n3).  its and v are HOST
 * arrays of n objects / device arrays.  Gathering across processes is the caller's. */
int cmdg_interp_scatter(cmdg_handle h, const cmdg_interp *its, int32_t n, const double *const *v,
                        int32_t nstate, double *fiv);
/* the finishing pass of the AtmosGCMDefault group (atmos_gcm_default.jl:375-379, :150-165) for the n
 * ranks of one process.  vG[r] (14, npoints_r) is the interpolated nodal array G of cmdg_gcm_nodal,
 * vB[r] (3, npoints_r) the interpolated VorticityModel tendency; neither is changed.  The triples rho u,
 * Omega and Omega_bl are projected with the expressions of cmdg_interp_project, u, v, w = rho u_i /
 * rho_i and et = rho e_i / rho_i are formed, and the 13 variables u, v, w, rho, temp, pres, thd, et,
 * ei, ht, hi, vort, vort2 are stored through the index triples: fiv is (n1, n2, n3, 13) column-major.
 * The objects must carry a latitude-longitude grid. */
int cmdg_interp_gcm_finish(cmdg_handle h, const cmdg_interp *its, int32_t n, const double *const *vG,
                           const double *const *vB, double *fiv);

/* ---- direct stiffness summation (src/Numerics/Mesh/DSS.jl) --------------------------------------
 * dss!(Q, grid) makes a DG field single-valued at the nodes elements share: every copy of a shared
 * vertex, edge node or face node is replaced by the sum over the copies.  The descriptor carries
 * the reference's own tables unchanged (Int64, 1-based, Julia's column-major layouts): of
 * grid.topology (Topologies.jl:810-988, :1687-1850) and of the grid (Grids.jl:640-745).  Every
 * pointer is a HOST pointer and need not outlive cmdg_dss_create, which checks the tables and
 * flattens them into groups of (element, node) members, one group per shared node.
 *
 * The kernel gathers a group's members in the reference's order, adds them starting from -0.0 and
 * writes the sum to every member: additions only (the library is built without contraction), no
 * atomics, so the result equals the reference's loops (dss3d_CPU!, DSS.jl:128-165) bit for bit and is
 * the same in every run.  That is race-free because no node is in two groups, which create checks.
 *
 * Refused at create (CMDG_ERR_INVALID, message in cmdg_last_error(h)): fewer than 3 points in the
 * vertical or 2 in the horizontal; Np nelem beyond 2^31 - 1; offsets that do not start at 1, decrease
 * or cut a record; an element, node, local vertex (1..8), local edge (1..12), local face (1..6), edge
 * orientation (1..2) or face orientation (1 or 3) out of range; a node that appears in two groups.
 *
 * cmdg_dss_create, cmdg_dss_destroy and cmdg_dss_apply take a handle or NULL under the rules written
 * at the interpolation entries above: with a handle the summation is enqueued on that handle's
 * compute stream, after any deferred CMDG_OPT_ASYNC_RUN run, and the call returns without waiting
 * (follow with cmdg_synchronize), as cmdg_filter_apply does; with NULL it runs on the default stream
 * of the device the object was created on and the call returns when it is done, which serves
 * polynomial orders no engine is compiled for, such as (4, 4, 5). */
/* (the object type is cmdg_dss_t: cmdg_dss is the call that is the reference's dss!) */
typedef struct cmdg_dss_s *cmdg_dss_t;
typedef struct cmdg_dss_desc {
    int32_t Nq[3];             /* polynomialorders(grid) .+ 1 */
    int64_t nelem;             /* length(topology.elems): real and ghost elements */
    int64_t nreal;             /* length(topology.realelems) */
    int64_t nvt;               /* length(vtconnoff) - 1 */
    const int64_t *vtconn;     /* pairs (local vertex, element) */
    const int64_t *vtconnoff;  /* nvt + 1 offsets into vtconn, 1-based */
    int64_t nedg;              /* length(edgconnoff) - 1 */
    const int64_t *edgconn;    /* triples (local edge, orientation, element) */
    const int64_t *edgconnoff; /* nedg + 1 offsets into edgconn, 1-based */
    int64_t nfc;               /* size(fcconn, 1) */
    const int64_t *fcconn;     /* (nfc, 5) column-major: face, element, neighbour's face, neighbour, orientation */
    const int64_t *vertmap;    /* 8 */
    const int64_t *edgemap;    /* (Nemax, 12, 2) column-major, -1 where an edge has fewer nodes */
    int64_t Nemax;             /* size(edgemap, 1) */
    const int64_t *facemap;    /* (Nfmax, 6, 2) column-major, -1 where a face has fewer nodes */
    int64_t Nfmax;             /* size(facemap, 1) */
} cmdg_dss_desc;
int cmdg_dss_create(cmdg_handle h, const cmdg_dss_desc *d, cmdg_dss_t *out);
/* waits for the handle h (if given) and for the device's default stream, then frees the tables; work
 * that used the object through ANOTHER handle must have been synchronised by the caller */
int cmdg_dss_destroy(cmdg_handle h, cmdg_dss_t dss);
/* out[0..3]: groups, members, the most members of one group, nodes touched */
int cmdg_dss_info(cmdg_dss_t dss, int64_t out[4]);
/* the summation alone, in place, on Q (Np, nstate, nelem) with nelem as at create (ghost elements
 * take part: they must hold their owners' values, as after a ghost exchange) */
int cmdg_dss_apply(cmdg_handle h, cmdg_dss_t dss, double *Q, int32_t nstate);
/* dss!(Q, grid) (DSS.jl:21-76): begin_ghost_exchange!, end_ghost_exchange! with unpacking into the
 * ghost elements -- the path of cmdg_halo_begin / cmdg_halo_end, so nstate beyond the handle's
 * exchange buffers is refused as there -- then the summation, ordered after the exchange.  Needs a
 * handle whose grid is the object's (same Np and element count); returns when the work is done. */
int cmdg_dss(cmdg_handle h, cmdg_dss_t dss, double *Q, int32_t nstate);
/* the same for handles connected with cmdg_comm_connect_local: begin on all, end on all, sum on all,
 * synchronise all.  dss and Q are HOST arrays of n objects / device arrays. */
int cmdg_group_dss(cmdg_handle *handles, int32_t n, const cmdg_dss_t *dss, double **Q, int32_t nstate);

/* ---- law-specific update_auxiliary_state! / update_auxiliary_state_gradient! ----------- */
/* Laws whose auxiliary state needs more than a nodal refresh override these two methods in
 * the reference (BalanceLaws/interface.jl:276-305; called at DGModel.jl:110-116,161-172 and
 * :210-222,355-361).  Their bodies are compositions of operators this library has; the hooks
 * record such a composition and the operator runs it at the reference's call sites:
 *   before the gradient pass (real elements): pre_filter[i] applied to Q
 *       -- HBModel: vertical cutoff filter on u, exponential filter on theta
 *          (hydrostatic_boussinesq_model.jl:654-680)
 *   after the gradient pass (real elements, and ghost elements once their gradient flux
 *   arrived):  aux[:, copy_aux_col[i]] = copy_scale[i] * gradflux[:, copy_gf_col[i]];
 *       upward column integral; downward column integral; aux[:, surf_dst_col[i]] over each
 *       stack = aux[:, surf_src_col[i]] at the top node of the stack
 *       -- HBModel: w = -div_h u, (w, pkin) integrals, wz0 (:693-726) */
#define CMDG_MAX_HOOK_OPS 4
typedef struct cmdg_rhs_hooks {
    int32_t npre;
    cmdg_filter pre_filter[CMDG_MAX_HOOK_OPS];
    int32_t ncopy;
    int32_t copy_gf_col[CMDG_MAX_HOOK_OPS], copy_aux_col[CMDG_MAX_HOOK_OPS];
    double copy_scale[CMDG_MAX_HOOK_OPS];
    int32_t has_integral, has_reverse_integral;
    cmdg_stack_integral_desc integral;         /* src/scale/dst: upward integral */
    cmdg_stack_integral_desc reverse_integral; /* rsrc/rdst: downward integral; both act on
                                                  the handle's state_auxiliary */
    int32_t nsurf;
    int32_t surf_src_col[CMDG_MAX_HOOK_OPS], surf_dst_col[CMDG_MAX_HOOK_OPS];
    int32_t nvertelem;
    const double *Imat; /* HOST (Nq, Nq) column-major grid.Imat[dim] */
    /* compute_flow_deviation!(dg, ::HBModel, ::Coupled, Q, t)
     * (src/Ocean/SplitExplicit/HydrostaticBoussinesqCoupling.jl:43-85), run after the pre
     * filters: aux[flow_ud_col + c] = Q[flow_u_col + c] - (1 / flow_H) * (column integral of
     * Q[flow_u_col + c]), c = 0, 1 */
    int32_t has_flow_deviation, flow_u_col, flow_ud_col;
    double flow_H;
    /* SplitExplicit01's OceanModel does everything in update_auxiliary_state!
     * (src/Ocean/SplitExplicit01/OceanModel.jl:432-541), i.e. BEFORE the gradient pass, and takes
     * the horizontal divergence from a DG operator of its own (Continuity3dModel):
     *   pre filters; pre_rhs_handle (if not NULL) is evaluated on Q with increment = false and
     *   column pre_rhs_src_col of its tendency goes to auxiliary column pre_rhs_dst_aux_col;
     *   then, with ops_before_gradients != 0, the integral / reverse integral / surface
     *   operations above run here instead of after the gradient pass; then the flow deviation.
     * Partitioned grids: the nested operator lives on the same partition (same neighbours) and
     * exchanges with its own communicator (RCCL: cmdg_comm_init_rccl on it too; local transport:
     * the nested operators form a group of their own, and cmdg_group_rhs runs them in lock step
     * between the two halves of the composition).  After the exchange of Q the operator repeats
     * the column operators over the received face pencils of the ghost stacks (the kinematic
     * pressure rank-boundary faces read on their plus side), as it does for the flow deviation.
     * Lifetime: the nested handle may be destroyed first -- cmdg_destroy detaches it from every
     * handle whose hooks name it; such a handle then fails every evaluation with CMDG_ERR_INVALID
     * ("the nested operator of this handle was destroyed") until cmdg_set_rhs_hooks gives it new
     * hooks (or NULL): it never goes on computing a different law. */
    int32_t ops_before_gradients;
    cmdg_handle pre_rhs_handle;
    int32_t pre_rhs_src_col, pre_rhs_dst_aux_col;
} cmdg_rhs_hooks;
/* hooks == NULL clears them.  Filters must outlive their use. */
int cmdg_set_rhs_hooks(cmdg_handle h, const cmdg_rhs_hooks *hooks);

/* ---- split-explicit ocean (src/Numerics/ODESolvers/SplitExplicitMethod.jl:1-177 and
 * src/Ocean/SplitExplicit/Communication.jl) --------------------------------------------
 * `slow` is the 3-D HydrostaticBoussinesqModel handle (Coupled), `fast` the ShallowWaterModel
 * handle on the one-layer extrusion of the 2-D grid; both share the horizontal element order
 * and the horizontal polynomial order.  Columns are 0-based; vector fields take two
 * consecutive columns. */
typedef struct cmdg_ocean_coupling_desc {
    int32_t nvertelem;  /* stack size of the slow grid */
    double H;           /* problem.H */
    const double *Imat; /* HOST (Nq, Nq) column-major vertical grid.Imat of the slow grid */
    int32_t slow_u_col, slow_eta_col;  /* slow state: u[2], eta */
    int32_t slow_dGu_col;              /* slow auxiliary: dG_u[2] */
    int32_t fast_eta_col, fast_U_col;  /* fast state: eta, U[2] */
    int32_t fast_GU_col, fast_du_col;  /* fast auxiliary: G_U[2], Delta_u[2] */
} cmdg_ocean_coupling_desc;
/* initialize_states! (Communication.jl:1-12): slow.aux.dG_u = -0 */
int cmdg_ocean_initialize_states(cmdg_handle slow, cmdg_handle fast,
                                 const cmdg_ocean_coupling_desc *d);
/* tendency_from_slow_to_fast! (Communication.jl:14-70): int du = column integral of the
 * slow tendency dQ_slow's u; fast.aux.G_U = int du, slow.aux.dG_u -= int du / H */
int cmdg_ocean_tendency_from_slow_to_fast(cmdg_handle slow, cmdg_handle fast,
                                          const cmdg_ocean_coupling_desc *d,
                                          const double *dQ_slow);
/* reconcile_from_fast_to_slow! (Communication.jl:100-170): fast.aux.Delta_u = 1/H (U - int u),
 * Q_slow.u += Delta_u through the column, Q_slow.eta = Q_fast.eta */
int cmdg_ocean_reconcile_from_fast_to_slow(cmdg_handle slow, cmdg_handle fast,
                                           const cmdg_ocean_coupling_desc *d, double *Q_slow,
                                           const double *Q_fast);
/* ---- the older split-explicit ocean, src/Ocean/SplitExplicit01 -------------------------
 * dostep!(Qvec, split::SplitExplicitLSRK2nSolver, param, time)
 * (SplitExplicitLSRK2nMethod.jl:81-190) with the exchange functions of
 * src/Ocean/SplitExplicit01/Communication.jl: per slow stage initialize_fast_state! (number and
 * size of the barotropic sub-steps, averaging window), initialize_adjustment!, the slow
 * right-hand side twice (increment = false for the barotropic forcing, increment = true for the
 * stage), tendency_from_slow_to_fast!, update!, the sub-steps with cummulate_fast_solution!,
 * reconcile_from_fast_to_slow!.  `slow` = CMDG_PHYSICS_OCEAN_SE01 with its hooks installed,
 * `fast` = CMDG_PHYSICS_BAROTROPIC_SE01 on the one-layer extrusion of the 2-D grid, created on
 * the same device (CMDG_ERR_INVALID otherwise).
 * numImplSteps > 0 (implicit vertical diffusion, IVDCModel.jl) is not carried. */
typedef struct cmdg_ocean01_desc {
    int32_t nvertelem;          /* stack size of the slow grid */
    double H;                   /* problem.H */
    const double *Imat;         /* HOST (Nq, Nq) column-major vertical grid.Imat of the slow grid */
    int32_t add_fast_substeps;  /* OceanModel.add_fast_substeps */
    /* the fast solver's own LSRK scheme (split.fast_solver, SplitExplicitLSRK2nMethod.jl:150-165):
     * nstages_fast > 0 with its three HOST coefficient arrays; 0 = the slow solver's scheme (the
     * reference's simple_box_2dt.jl builds both solvers from LSRK54CarpenterKennedy) */
    int32_t nstages_fast;
    const double *rka_fast, *rkb_fast, *rkc_fast;
} cmdg_ocean01_desc;
int cmdg_split_explicit01_step(cmdg_handle slow, cmdg_handle fast, const cmdg_ocean01_desc *d,
                               double *Q3, double *dQ3, double *dQ2fast, double *Q2, double *dQ2,
                               double t, double dt, double dt_fast, int32_t nstages,
                               const double *rka, const double *rkb, const double *rkc);
/* the same step for the n (slow, fast) pairs of one process whose slow models, fast models and
 * nested continuity operators are each connected by cmdg_comm_connect_local (pair i = rank i);
 * with the RCCL transport every rank calls cmdg_split_explicit01_step on its own pair */
int cmdg_group_split_explicit01_step(cmdg_handle *slow, cmdg_handle *fast, int32_t n,
                                     const cmdg_ocean01_desc *d, double **Q3, double **dQ3,
                                     double **dQ2fast, double **Q2, double **dQ2, double t, double dt,
                                     double dt_fast, int32_t nstages, const double *rka,
                                     const double *rkb, const double *rkc);

/* update!() of the LSRK methods on the handle's real elements (LowStorageRungeKuttaMethod.jl:
 * 146-166): Q += rkb_dt * dQ; dQ *= rka_next */
int cmdg_lsrk_update(cmdg_handle h, double *dQ, double *Q, double rka_next, double rkb_dt);
/* lsrk_mri_update!() of the LSRK methods as the fast solver of an MRI-GARK scheme
 * (LowStorageRungeKuttaMethod.jl:206-225) on the handle's real elements:
 * dq = dQ + sc[0] R[0] + ... + sc[nR-1] R[nR-1] (in that order); Q += rkb_dt dq; dQ = rka_next dq.
 * R: HOST array of nR device arrays shaped like Q, 1 <= nR <= CMDG_MRI_MAXR; sc: HOST array of
 * nR scalars (the reference's Horner sums in tau, computed by the caller).  Enqueued on the
 * handle's stream; no copy to the device, no host wait. */
#define CMDG_MRI_MAXR 6
int cmdg_mri_lsrk_update(cmdg_handle h, double *dQ, double *Q, double rka_next, double rkb_dt, int32_t nR,
                         const double *const *R, const double *sc);
/* mri_create_Qhat! (MultirateInfinitesimalGARKDecoupledImplicit.jl:220-237) on the handle's real
 * elements: Qhat = Q + sc[0] R[0] + ... + sc[nR-1] R[nR-1]; R and sc as above */
int cmdg_mri_qhat(cmdg_handle h, double *Qhat, const double *Q, int32_t nR, const double *const *R,
                  const double *sc);
/* dostep!(Q, ssp::StrongStabilityPreservingRungeKutta, p, time)
 * (src/Numerics/ODESolvers/StrongStabilityPreservingRungeKuttaMethod.jl:117-165, update! kernel
 * :167-190): Qstage = Q; per stage Rstage = rhs(Qstage, t + rkc[s] dt) (increment = false) and
 * Qstage = rka[2 s] Q + rka[2 s + 1] Qstage + dt rkb[s] Rstage; finally Q = Qstage.  rka is the
 * (nstages, 2) coefficient matrix row-major; Rstage and Qstage are caller-owned arrays of Q's
 * shape. */
int cmdg_ssprk_step(cmdg_handle h, double *Q, double *Rstage, double *Qstage, double t, double dt,
                    int32_t nstages, const double *rka, const double *rkb, const double *rkc);

/* dostep!(Q, lsrk3n::LowStorageRungeKutta3N, p, time)
 * (src/Numerics/ODESolvers/LowStorageRungeKutta3NMethod.jl:153-226, Fyfe 1966): dR = -0; per
 * stage dQ += rhs(Q, t + rkc[s] dt), then Q += rkb[2 s] dt dQ + rkb[2 s + 1] dt dR,
 * dR += rka[2 s' + 1] dQ, dQ *= rka[2 s'] with s' = (s + 1) mod nstages.  rka and rkb are the
 * (nstages, 2) matrices row-major; dQ (zero before the first step) and dR are caller-owned
 * arrays of Q's shape. */
int cmdg_ls3n_step(cmdg_handle h, double *Q, double *dQ, double *dR, double t, double dt,
                   int32_t nstages, const double *rka, const double *rkb, const double *rkc);

/* dostep!(Qslow, split::SplitExplicitSolver, param, time) (SplitExplicitMethod.jl:70-177): one
 * slow step of size dt_slow whose every stage sub-steps the fast model with full LSRK steps
 * of at most dt_fast.  dQ_slow / dQ_fast are the LSRK tendency accumulators (zero before the
 * first step), dQ2fast a scratch of the slow state's shape.  coupled == 0 runs the two
 * models side by side without the exchange (the `Uncoupled` variant of the test). */
int cmdg_split_explicit_step(cmdg_handle slow, cmdg_handle fast,
                             const cmdg_ocean_coupling_desc *d, int32_t coupled, double *Q_slow,
                             double *dQ_slow, double *dQ2fast, double *Q_fast, double *dQ_fast,
                             double t, double dt_slow, double dt_fast, int32_t nstages,
                             const double *rka, const double *rkb, const double *rkc);

/* the same step for n (slow, fast) pairs connected by cmdg_comm_connect_local (slow handles
 * among themselves, fast handles among themselves), driven in lock step by one host thread; the
 * element partition keeps whole columns, and slow[i] / fast[i] own the same columns */
int cmdg_group_split_explicit_step(cmdg_handle *slow, cmdg_handle *fast, int32_t n,
                                   const cmdg_ocean_coupling_desc *d, int32_t coupled,
                                   double **Q_slow, double **dQ_slow, double **dQ2fast,
                                   double **Q_fast, double **dQ_fast, double t, double dt_slow,
                                   double dt_fast, int32_t nstages, const double *rka,
                                   const double *rkb, const double *rkc);

/* ---- measurement --------------------------------------------------------------- */
enum {
    CMDG_K_GRADIENTS = 0, CMDG_K_DIVGRAD = 1, CMDG_K_GRADLAP = 2, CMDG_K_TENDENCY = 3,
    CMDG_K_PACK = 4, CMDG_K_UNPACK = 5, CMDG_K_UPDATE_AUX = 6, CMDG_K_FILTER = 7,
    CMDG_K_STACK_INTEGRAL = 8,
    /* halo: the transport between pack and unpack (RCCL group or device copies) on the halo
     * stream, and the time the compute stream had to wait for an exchange to finish (the part of
     * an exchange NOT hidden behind interior work; one record per exchange, zero when hidden) */
    CMDG_K_TRANSPORT = 9, CMDG_K_HALO_EXPOSED = 10,
    /* the exterior launches of the four passes of a handle with neighbours (their interior
     * launches stay under CMDG_K_GRADIENTS ... CMDG_K_TENDENCY) */
    CMDG_K_GRADIENTS_EXT = 11, CMDG_K_DIVGRAD_EXT = 12, CMDG_K_GRADLAP_EXT = 13,
    CMDG_K_TENDENCY_EXT = 14,
    /* the vertical finite-volume passes of a DGFVModel handle (interior and exterior launches) */
    CMDG_K_FV_GRADIENTS = 15, CMDG_K_FV_TENDENCY = 16,
    /* the flux-differencing launch of an ESDGModel handle (interior and exterior launches) */
    CMDG_K_ESDG_TENDENCY = 17, CMDG_K_COUNT = 18
};
/* bracket every launch with HIP events on the launch stream (off by default) */
int cmdg_profile_enable(cmdg_handle h, int32_t on);
int cmdg_profile_get(cmdg_handle h, int32_t kernel, double *total_ms, int64_t *launches);
int cmdg_profile_reset(cmdg_handle h);

/* ---- ManyColumnLU and the IMEX step (columnwise_lu_solver.jl, AdditiveRungeKuttaMethod.jl) ----
 * A column solver owns the banded matrix I - alpha L of every column of a VerticalDirection DG
 * model `linear` on a stacked grid (CMDG_PHYSICS_ATMOS_LINEAR_AG or
 * CMDG_PHYSICS_ESDG_DRY_ATMOS_LINEAR_AG with nstate = 5, CMDG_PHYSICS_MOIST_LINEAR_AG with nstate = 6; eband = 1, bandwidths p = q = Nq_v nstate - 1;
 * compiled for (N, nstate) = (3, 5), (4, 5), (5, 5), (4, 6), (6, 6)).  A column is one horizontal node of one stack of `nvertelem` elements;
 * the real elements must be whole stacks, bottom first.  Every stack must end in boundary faces:
 * a vertically periodic stack (no boundary face at the bottom of its first or the top of its last
 * element) is refused with CMDG_ERR_UNSUPPORTED, since the band cannot hold the coupling of its
 * top and bottom elements.  Assembly probes `linear` (3 Nq_v nstate
 * evaluations at t = NaN, update_banded_matrix!); factorisation is band_lu! without pivoting.
 * The band lives on the device, ncol n (p + q + 1) doubles: cmdg_columnlu_create refuses
 * (CMDG_ERR_INVALID, message naming the size) when that does not fit in free device memory.
 * Errors are reported through cmdg_last_error(linear).  The solver is driven on linear's stream. */
typedef struct cmdg_columnlu *cmdg_columnlu_handle;
/* assemble I - alpha L and factor it (prefactorize(EulerOperator(f, -alpha), ManyColumnLU(), ...)) */
int cmdg_columnlu_create(cmdg_handle linear, int32_t nvertelem, double alpha, cmdg_columnlu_handle *out);
/* reassemble and refactor for a new alpha (update_backward_Euler_solver!, isadjustable = true) */
int cmdg_columnlu_update(cmdg_columnlu_handle lu, double alpha);
/* assemble I - alpha L only, unfactored (for cmdg_columnlu_export_band; a solve then refuses) */
int cmdg_columnlu_assemble(cmdg_columnlu_handle lu, double alpha);
/* Q = (I - alpha L)^-1 Qrhs, both (Np, nstate, nelem) device arrays, real elements; Q may be Qrhs */
int cmdg_columnlu_solve(cmdg_columnlu_handle lu, double *Q, const double *Qrhs);
/* out[8] = n, p, q, ncol, band bytes, state (1 assembled, 2 factored), nvertelem, Nq_v */
int cmdg_columnlu_info(cmdg_columnlu_handle lu, int64_t *out);
/* the alpha the band was last assembled for */
int cmdg_columnlu_alpha(cmdg_columnlu_handle lu, double *alpha);
/* HOST out[n (p + q + 1)]: the band of column `column` (horizontal node i + Nq j of stack h is
 * column h Nq^2 + i + Nq j, all 0-based) in the reference's layout, A[d, col] at out[col (p + q + 1)
 * + d] with d = row - col + q: the assembled operator or its LU factors, whichever it holds now */
int cmdg_columnlu_export_band(cmdg_columnlu_handle lu, int64_t column, double *out);
int cmdg_columnlu_destroy(cmdg_columnlu_handle lu);
/* One step of a low-storage additive Runge-Kutta method (dostep!(..., ::LowStorageVariant),
 * AdditiveRungeKuttaMethod.jl:415-523) with the explicit operator `full` and the implicit one the
 * solver's `linear`: tableaus row-major (nstages, nstages), 2 <= nstages <= 4, the implicit diagonal
 * (0, c, ..., c).  work: 2 nstages + 1 device state arrays shaped like Q (Qstages[2..], Rstages,
 * Qhat, Qtt).  split_explicit_implicit != 0: the explicit operator is full minus linear,
 * evaluated as `full` followed by `linear` with alpha = -1 and increment.  The solver is refactored
 * when dt a_ii differs from its alpha.  `full` and `linear` have the same state count, or `linear`
 * ends before trailing states of `full` that the linear model does not carry (the tracers of
 * CMDG_PHYSICS_DRY_ATMOS, iparam[15] bits 8..15; AtmosModel.jl:399-406): work then holds four more
 * arrays shaped like the linear handle's state, the leading columns are moved in and out of them,
 * the trailing states are stepped explicitly and the column solver's band is that of the model
 * without them.  Any other pair of counts is CMDG_ERR_INVALID, as is such a pair with GMRES or with
 * an ESDGModel.  `full` may be an ESDGModel handle (cmdg_create_esdg) with
 * CMDG_PHYSICS_ESDG_DRY_ATMOS_LINEAR_AG as `linear`, on one rank (CMDG_ERR_UNSUPPORTED with ghost
 * elements).  A failure's message is on both handles.  Returns after the step has finished. */
int cmdg_ark_step(cmdg_handle full, cmdg_columnlu_handle lu, double *Q, double *const *work, double t,
                  double dt, int32_t nstages, const double *rka_explicit, const double *rka_implicit,
                  const double *rkb, const double *rkc, int32_t split_explicit_implicit);

/* ---- GeneralizedMinimalResidual (generalized_minimal_residual_solver.jl, linearsolve!) ----------
 * Restarted GMRES for (I - alpha L) Q = Qrhs, L any handle cmdg_rhs serves, in any direction, on a
 * stacked or unstacked grid, single rank.  initialize!: r0 = Qrhs - A Q from the caller's Q,
 * threshold = rtol |r0|; threshold < atol returns converged after 0 iterations with Q untouched,
 * otherwise the working threshold is max(threshold, atol).  Cycles of at most M Arnoldi steps
 * (modified Gram-Schmidt, one Givens rotation per column) break when |g0[j+1]| < threshold; after a
 * cycle Q += sum y_i v_i and, when not converged, the solver restarts from the new residual.  At
 * most max_iters inner iterations in total.  Dots and norms are plain sums over the real elements
 * (weighted_norm = false), accumulated in fp64 in a fixed order: a repeated solve repeats its bits.
 * The solver owns M + 1 device arrays shaped like Q and its small matrices; one host wait per inner
 * iteration reads the residual norm.  Refused at create, message in cmdg_last_error(linear):
 * CMDG_ERR_INVALID for M outside 1 .. CMDG_GMRES_MAX_M, rtol or atol negative or NaN, or a basis
 * that does not fit in free device memory (the message names its size); CMDG_ERR_UNSUPPORTED for a
 * handle with halo neighbours (a multi-rank solve needs an all-reduce per dot and one convergence
 * decision for every rank: a follow-up). */
#define CMDG_GMRES_MAX_M 64
typedef struct cmdg_gmres *cmdg_gmres_handle;
typedef struct cmdg_gmres_info {
    int64_t iterations;    /* inner iterations done */
    int32_t converged;
    double residual_norm;  /* |g0[j+1]| of the last iteration; |r0| after 0 iterations */
    double threshold;      /* the working threshold */
} cmdg_gmres_info;
int cmdg_gmres_create(cmdg_handle linear, int32_t M, double rtol, double atol, cmdg_gmres_handle *out);
/* the size check of cmdg_gmres_create against free_bytes of device memory (CMDG_ERR_INVALID and the
 * message when the basis does not fit); basis_bytes (may be NULL) receives (M + 1) state arrays */
int cmdg_gmres_fits(cmdg_handle linear, int32_t M, int64_t free_bytes, int64_t *basis_bytes);
/* setup_backward_Euler_solver / update_backward_Euler_solver!: the alpha the step entries compare
 * with dt a_ii (prefactorize does nothing for an iterative solver) */
int cmdg_gmres_prepare(cmdg_gmres_handle g, double alpha);
/* Q: initial guess in, solution out; Q and Qrhs are distinct device arrays shaped like the linear
 * handle's state; t is passed to L; max_iters < 0: the reference's default, the length of Q.  A
 * solve that stops at max_iters returns CMDG_OK with info->converged = 0.  A residual norm that is
 * not finite is CMDG_ERR_INVALID with a message. */
int cmdg_gmres_solve(cmdg_gmres_handle g, double alpha, double *Q, const double *Qrhs, double t,
                     int64_t max_iters, cmdg_gmres_info *info);
/* the solves of the last cmdg_ark_step_gmres / cmdg_mrigark_step_gmres, in order: *nsolves of them,
 * the first min(capacity, *nsolves) copied to out */
int cmdg_gmres_step_info(cmdg_gmres_handle g, int32_t capacity, cmdg_gmres_info *out, int32_t *nsolves);
int cmdg_gmres_destroy(cmdg_gmres_handle g);
/* cmdg_ark_step with GMRES as the backward-Euler solver: `linear` is the solver's handle, of any
 * direction; Qtt is initialised to Qhat by the stage update (the solver's initial guess,
 * AdditiveRungeKuttaMethod.jl:603); every solve runs with max_iters = the length of Q */
int cmdg_ark_step_gmres(cmdg_handle full, cmdg_gmres_handle gmres, double *Q, double *const *work, double t,
                        double dt, int32_t nstages, const double *rka_explicit, const double *rka_implicit,
                        const double *rkb, const double *rkc, int32_t split_explicit_implicit);

/* One slow step of a multirate infinitesimal GARK scheme (Sandu 2019) whose fast method is a
 * low-storage 2N Runge-Kutta method: dostep! of MultirateInfinitesimalGARKExplicit.jl (kind
 * CMDG_MRIGARK_EXPLICIT) or of MultirateInfinitesimalGARKDecoupledImplicit.jl (kind
 * CMDG_MRIGARK_DECOUPLED_IMPLICIT).  Each slow stage s evaluates the slow operator into
 * Rstages[s], then runs the fast solve! loop from the stage time ts to ts + dc[s] dt with the
 * fast dt, the last fast step shortened to end there (adjustfinalstep); every fast stage is one
 * evaluation of the fast operator (increment) and one k_lsrk_mri_update.  The decoupled-implicit
 * kind then forms Qhat (k_mri_qhat) and solves (I - alpha L) Q = Qhat with the column solver,
 * alpha = dt gamma[0][2s+1][s+1]: when alpha differs from the solver's the solver is refactored
 * if lu_adjustable, and the step is refused (CMDG_ERR_INVALID) otherwise. */
#define CMDG_MRIGARK_EXPLICIT 0
#define CMDG_MRIGARK_DECOUPLED_IMPLICIT 1
#define CMDG_MRI_MAXGAMMA 4
typedef struct cmdg_mrigark_desc {
    int32_t kind;
    int32_t nstages;  /* slow stages, 1 .. CMDG_MRI_MAXR */
    int32_t ngamma;   /* coupling matrices Gamma_0 .. Gamma_{ngamma-1}, 1 .. CMDG_MRI_MAXGAMMA */
    /* HOST, ngamma row-major matrices: explicit (nstages, nstages) holding Gamma_k ./ dc;
     * decoupled implicit (2 nstages, nstages + 1) holding Gamma_k as given */
    const double *gamma;
    const double *dc;  /* HOST nstages: the explicit stages' time fractions */
    int32_t fast_nstages;  /* the fast 2N tableau, 1 .. 14 stages */
    const double *fast_rka, *fast_rkb, *fast_rkc;  /* HOST */
    double fast_dt;
    int32_t lu_adjustable;  /* decoupled implicit: LinearBackwardEulerSolver's isadjustable */
} cmdg_mrigark_desc;
/* The slow operator is `slow`, or `slow` minus `slow_minus` when that is not NULL (a remainder,
 * evaluated as `slow` then `slow_minus` with alpha = -1 and increment); the same for `fast` and
 * `fast_minus`.  All handles live on one grid with one state count.  lu: required for the
 * decoupled-implicit kind, whose slow operator must be lu's linear model (no remainder), and NULL
 * for the explicit kind.  work: HOST array of device arrays shaped like Q: Rstages[nstages], the
 * fast dQ (zero on entry, zero again on return), Qhat (decoupled implicit only).  Refusals
 * (CMDG_ERR_INVALID, the message naming the member): another grid or state count, nstages or
 * ngamma out of range, a fast tableau longer than 14 stages, dt <= 0, fast_dt <= 0, a missing lu
 * or work array.  Returns after the step has finished. */
int cmdg_mrigark_step(cmdg_handle slow, cmdg_handle slow_minus, cmdg_handle fast, cmdg_handle fast_minus,
                      cmdg_columnlu_handle lu, const cmdg_mrigark_desc *d, double *Q, double *const *work,
                      double t, double dt);
/* the decoupled-implicit kind with GMRES in place of the column solver (required): the slow
 * operator is the solver's linear handle, in any direction; Q is each solve's initial guess */
int cmdg_mrigark_step_gmres(cmdg_handle slow, cmdg_handle slow_minus, cmdg_handle fast, cmdg_handle fast_minus,
                            cmdg_gmres_handle gmres, const cmdg_mrigark_desc *d, double *Q,
                            double *const *work, double t, double dt);

/* ---- AtmosLESDefault diagnostics (src/Diagnostics/atmos_les_default.jl) ------------------------
 * Density-weighted horizontal means, variances and vertical eddy fluxes per level of a stacked
 * grid, plus the cloud statistics of the moist law, formed on the device.  Levels: L = Nqk *
 * nvertelem, evk = Nqk (ev - 1) + k, element e = ev + (eh - 1) nvertelem (helpers.jl:6-28).  Served
 * for the dry atmosphere law in its LES configurations (flat orientation, no hyperdiffusion) and
 * the moist law; any other law, a grid that is not stacked and a vertical order of 0 are refused
 * (CMDG_ERR_UNSUPPORTED / CMDG_ERR_INVALID with a message).
 *
 * Every level sum is accumulated in double-double from terms that are the correctly rounded double
 * expressions the reference writes, partials are combined in a fixed order (work-group, then rank),
 * and the returned sum is the double nearest to the double-double: two calls on the same input
 * return the same bits.  The calls read aux.moisture and the gradient flux as the last evaluation
 * of the handle left them: evaluate the handle at (Q, t) first where they must belong to Q. */
/* out[4] = ndiag (nodal columns), nsimple (13 / 20), nho (11 / 21), nlevels */
int cmdg_les_query(cmdg_handle h, int32_t nvertelem, int32_t *out);
/* the nodal pass alone: D is a DEVICE array (ndiag, Np, nelem), its real elements are written.
 * Columns: temp, pres, theta_dry, e_int, h_tot, h_int, d_h_tot[3]; the moist law adds q_liq, q_ice,
 * q_vap, theta_vir, theta_liq_ice, has_condensate (0.0 / 1.0), d_q_tot[3].  Returns when D is ready. */
int cmdg_les_nodal(cmdg_handle h, const double *Q, double t, double *D);
/* atmos_collect_onetime (atmos_common.jl:12-38): HOST zvals[L] (x3 of the last node this rank
 * visits on the level) and MH_z[L] (the level's sum of MH over all ranks).  Required once before
 * cmdg_les_collect; a handle with an RCCL communicator combines across ranks (collective).
 * omega: HOST, the Nqk quadrature weights of the vertical direction (grid.omega[end]) for the
 * water paths, Mvert = omega_k JcV[1, k, ev, eh = 1] (:781-790); NULL: lwp and iwp come out 0. */
int cmdg_les_init(cmdg_handle h, int32_t nvertelem, const double *omega, double *zvals, double *MH_z);
/* HOST arrays of one collection, row-major; a NULL member is not written */
typedef struct cmdg_les_result {
    double *simple_sums;   /* (L, nsimple) the sums of atmos_les_default_simple_sums! */
    double *simple_avgs;   /* (L, nsimple) ... / MH_z, and all but avg_rho / avg_rho */
    double *ho_sums;       /* (L, nho) the sums of atmos_les_default_ho_sums! about simple_avgs */
    double *ho_avgs;       /* (L, nho) ... / MH_z / avg_rho */
    /* moist law only (untouched otherwise).  cloud_levels (L, 6): nodes with condensate, nodes,
     * sum MH q_liq rho rho, sum MH q_ice rho rho, and those two / MH_z / avg_rho.  cloud_scalars
     * [8]: cld_top, cld_base (NaN without condensate), cld_cover, lwp, iwp, node columns with
     * condensate, node columns, 0. */
    double *cloud_levels;
    double *cloud_scalars;
} cmdg_les_result;
/* atmos_les_default_collect (:567-871) at (Q, t).  Without a communicator everything up to the final
 * copy-out is enqueued on the compute stream; with an RCCL communicator the ranks' double-double
 * partials are gathered and combined in rank order on every rank (collective).  Returns when the
 * results are on the host. */
int cmdg_les_collect(cmdg_handle h, const double *Q, double t, const cmdg_les_result *out);
/* ... for handles connected with cmdg_comm_connect_local (handle i = rank i): zvals are rank 0's;
 * Q: HOST array of n device arrays */
int cmdg_group_les_init(cmdg_handle *handles, int32_t n, int32_t nvertelem, const double *omega, double *zvals,
                        double *MH_z);
int cmdg_group_les_collect(cmdg_handle *handles, int32_t n, const double *const *Q, double t,
                           const cmdg_les_result *out);

/* ---- AtmosGCMDefault diagnostics (src/Diagnostics/atmos_gcm_default.jl, diagnostic_fields.jl) ---
 * Served for cmdg_create handles of laws whose state begins rho, rho u[3] (the dry and the moist
 * atmosphere); any other law, a DGFVModel handle (vertical order 0) and an ESDGModel handle are
 * refused with CMDG_ERR_UNSUPPORTED and the reason.  Arrays are DEVICE arrays in the layout of a
 * state; the calls return when their output is ready.
 * VectorGradients(dg, Q): vgrad (Np, 9, nreal), columns d1 u1, d2 u1, d3 u1, d1 u2, ... of u = rho u /
 * rho, with the reference's arithmetic (every sum left to right over rounded products). */
int cmdg_vector_gradients(cmdg_handle h, const double *Q, double *vgrad);
/* Vorticity(dg, vgrad): vort (Np, 3, nreal) = (d2 u3 - d3 u2, d3 u1 - d1 u3, d1 u2 - d2 u1) */
int cmdg_vorticity(cmdg_handle h, const double *vgrad, double *vort);
/* the nodal pass of the group in one launch: G (Np, 14, nelem) = rho, rho u[3], rho e | temp, pres,
 * theta_dry, e_int, h_tot, h_int of compute_thermo! (thermo.jl:33-44) | Omega[3], and u (Np, 3, nelem),
 * the auxiliary array of the group's CMDG_PHYSICS_VORTICITY handle; real elements are written.  Bit for
 * bit the columns of the separate calls.  The dry atmosphere law with an orientation; the moist law
 * is refused (its columns are not built). */
int cmdg_gcm_nodal(cmdg_handle h, const double *Q, double t, double *G, double *u);

#ifdef __cplusplus
}
#endif
#endif /* CMDG_H */
