// libcmdg: which engine serves a descriptor -- the table of the laws compiled in, the plug-in loader,
// cmdg_create / cmdg_create_dgfv / cmdg_create_esdg, cmdg_destroy and cmdg_last_error.
#include <dlfcn.h>

#include <algorithm>
#include <new>

#include "engine_base.h"
#include "laws.h"
#include "diagnostics.h"
#include "reductions.h"

using namespace cmdg;

static thread_local std::string g_create_err;
void cmdg::set_create_err(const std::string &msg) { g_create_err = msg; }

// ---- the laws compiled in: physics id -> factory, counts.  cmdg_physics_counts and cmdg_create look a law
// up here; the functions are defined per physics family in the engine_*.hip units (laws.h).
namespace {
struct Law {
    int32_t id;
    EngineBase *(*make)(const cmdg_desc *, std::string &);  // NULL: not a DGModel law (cmdg_create_esdg)
    int (*counts)(const int32_t *iparam, int32_t out[6]);
};
const Law LAWS[] = {
    {CMDG_PHYSICS_ADVECTION_DIFFUSION, make_engine_advdiff, counts_advdiff},
    {CMDG_PHYSICS_DRY_ATMOS, make_engine_atmos, counts_atmos},
    {CMDG_PHYSICS_HYDROSTATIC_BOUSSINESQ, make_engine_ocean, counts_ocean},
    {CMDG_PHYSICS_PRESSURE_GRADIENT, make_engine_pgrad, counts_pgrad},
    {CMDG_PHYSICS_SHALLOW_WATER, make_engine_sw, counts_sw},
    {CMDG_PHYSICS_MOIST_ATMOS, make_engine_moist, counts_moist},
    {CMDG_PHYSICS_OCEAN_SE01, make_engine_se01, counts_ocean_se01},
    {CMDG_PHYSICS_CONTINUITY3D_SE01, make_engine_se01, counts_continuity3d_se01},
    {CMDG_PHYSICS_BAROTROPIC_SE01, make_engine_se01, counts_barotropic_se01},
    {CMDG_PHYSICS_ATMOS_LINEAR_AG, make_engine_atmos_linear, counts_atmos_linear},
    {CMDG_PHYSICS_MOIST_LINEAR_AG, make_engine_moist_linear, counts_moist_linear},
    {CMDG_PHYSICS_ESDG_DRY_ATMOS, nullptr, counts_esdg_dryatmos},
    {CMDG_PHYSICS_ATMOS_LINEAR_ACOUSTIC, make_engine_atmos_acoustic, counts_atmos_acoustic},
    {CMDG_PHYSICS_ESDG_DRY_ATMOS_LINEAR_AG, make_engine_esdg_dryatmos_linear, counts_esdg_dryatmos_linear},
    {CMDG_PHYSICS_VORTICITY, make_engine_vorticity, counts_vorticity},
};
const Law *find_law(int32_t physics_id)
{
    for (const Law &l : LAWS)
        if (l.id == physics_id) return &l;
    return nullptr;
}
}  // namespace

// ---- engine plug-ins: balance-law functors / template combinations outside the compiled set ----
// A plug-in is a shared object built from this library's own headers (csrc/engine.h + a
// physics_*.h, one translation unit instantiating make_engine<Law, Nq>) that exports
//   cmdg::EngineBase *cmdg_plugin_make_engine(const cmdg_desc *, char *err, int errlen)
// returning NULL for a descriptor it does not serve.  climatemachine.jl_amd/plugins.py writes and
// builds them with hipcc (the reference compiles a law's pointwise functions into its kernels when
// the model is first run; this is the ahead-of-time equivalent for a C ABI).
namespace {
typedef EngineBase *(*plugin_make_t)(const cmdg_desc *, char *, int);
std::vector<plugin_make_t> g_plugin_make;
std::vector<std::string> g_plugin_path;
bool g_plugins_env_read = false;
int load_plugin(const char *path, std::string &err)
{
    for (const auto &p : g_plugin_path)
        if (p == path) return CMDG_OK;
    void *lib = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!lib) {
        err = std::string("cannot load plug-in: ") + dlerror();
        return CMDG_ERR_INVALID;
    }
    plugin_make_t f = (plugin_make_t)dlsym(lib, "cmdg_plugin_make_engine");
    if (!f) {
        err = std::string(path) + " does not export cmdg_plugin_make_engine";
        dlclose(lib);
        return CMDG_ERR_INVALID;
    }
    // a plug-in shares the C++ layout of EngineBase with the library: one built against other
    // headers is refused here instead of corrupting a handle later
    typedef unsigned long (*plugin_abi_t)();
    plugin_abi_t abi = (plugin_abi_t)dlsym(lib, "cmdg_plugin_abi");
    if (!abi || abi() != engine_abi_stamp()) {
        err = std::string(path) + (abi ? " was built against another libcmdg (engine layout differs): rebuild it"
                                       : " does not export cmdg_plugin_abi");
        dlclose(lib);
        return CMDG_ERR_INVALID;
    }
    g_plugin_make.push_back(f);
    g_plugin_path.push_back(path);
    return CMDG_OK;
}
EngineBase *plugin_engine(const cmdg_desc *d, std::string &err)
{
    if (!g_plugins_env_read) {
        g_plugins_env_read = true;
        if (const char *env = getenv("CMDG_PLUGINS")) {
            std::string all(env), e2;
            size_t a = 0;
            while (a <= all.size()) {
                const size_t b = all.find(':', a);
                const std::string one = all.substr(a, b == std::string::npos ? std::string::npos : b - a);
                if (!one.empty() && load_plugin(one.c_str(), e2) != CMDG_OK) err += e2 + "; ";
                if (b == std::string::npos) break;
                a = b + 1;
            }
        }
    }
    for (plugin_make_t f : g_plugin_make) {
        char buf[512] = {0};
        if (EngineBase *e = f(d, buf, (int)sizeof(buf))) return e;
        if (buf[0]) err += std::string(buf) + "; ";
    }
    if (g_plugin_make.empty() && err.empty()) err = "none loaded";
    return nullptr;
}
}  // namespace


extern "C" {

int cmdg_load_plugin(const char *path)
{
    if (!path) return CMDG_ERR_INVALID;
    std::string err;
    const int r = load_plugin(path, err);
    if (r) g_create_err = err;
    return r;
}

int cmdg_physics_counts(int32_t physics_id, const int32_t *iparam, int32_t out[6])
{
    if (!iparam || !out) return CMDG_ERR_INVALID;
    const Law *law = find_law(physics_id);
    return law ? law->counts(iparam, out) : CMDG_ERR_UNSUPPORTED;
}

int cmdg_atmos_host_constants(const int32_t *iparam, const double *dparam, double out[7])
{
    if (!iparam || !dparam || !out) return CMDG_ERR_INVALID;
    return host_constants_atmos(iparam, dparam, out);
}

static int create_handle(const cmdg_desc *d, const cmdg_fv_desc *fv, cmdg_handle *out, const cmdg_esdg_desc *esdg = nullptr)
{
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        g_create_err = "no HIP device visible";
        return CMDG_ERR_NO_DEVICE;
    }
    if (d->dim != 3 || d->N[0] != d->N[1]) {
        g_create_err = "only dim == 3 with one horizontal polynomial order is compiled in";
        return CMDG_ERR_UNSUPPORTED;
    }
    if (d->nf_first < CMDG_RUSANOV || d->nf_first > CMDG_ROE_MOIST_LVPP) {
        g_create_err = "unknown first-order numerical flux";
        return CMDG_ERR_INVALID;
    }
    if (d->nf_first >= CMDG_ROE && d->nf_first <= CMDG_LMARS && d->physics_id != CMDG_PHYSICS_DRY_ATMOS) {
        g_create_err = "Roe / HLLC / LMARS numerical fluxes are methods of the dry atmosphere law only";
        return CMDG_ERR_UNSUPPORTED;
    }
    if (d->nf_first >= CMDG_ROE_MOIST && d->physics_id != CMDG_PHYSICS_MOIST_ATMOS) {
        g_create_err = "RoeNumericalFluxMoist is a method of the moist atmosphere law (EquilMoist) only";
        return CMDG_ERR_UNSUPPORTED;
    }
    std::string err;
    EngineBase *e = nullptr;
    if (esdg) {
        e = make_engine_esdg(d, esdg, err);
        if (!e) {
            g_create_err = err;
            return CMDG_ERR_UNSUPPORTED;
        }
    } else if (fv) {
        if (d->physics_id == CMDG_PHYSICS_ADVECTION_DIFFUSION)
            e = make_engine_advdiff_fv(d, fv, err);
        else if (d->physics_id == CMDG_PHYSICS_DRY_ATMOS)
            e = make_engine_atmos_fv(d, fv, err);
        else  // (text pinned by tests/test_gpu_create_refusals.py; the dry atmosphere law is served above)
            err = "cmdg_create_dgfv: the finite-volume passes are compiled for the AdvectionDiffusion law only";
        if (!e) {
            g_create_err = err;
            return CMDG_ERR_UNSUPPORTED;
        }
    } else if (const Law *law = find_law(d->physics_id); law && law->make) {
        e = law->make(d, err);
    } else {
        err = "unknown physics_id";
    }
    if (!e) {  // not compiled in: ask the plug-ins (cmdg_load_plugin / CMDG_PLUGINS)
        std::string perr;
        e = plugin_engine(d, perr);
        if (!e) {
            g_create_err = perr.empty() ? err : err + "; plug-ins: " + perr;
            return CMDG_ERR_UNSUPPORTED;
        }
    }
    int r = e->init(d);
    if (r == CMDG_OK && fv) r = e->init_fv();
    if (esdg) e->reference_halo = true;  // the face phase reads ghost neighbours from the ghost elements
    if (r != CMDG_OK) {
        g_create_err = e->err;
        delete e;
        return r;
    }
    cmdg_context *c = new (std::nothrow) cmdg_context();
    if (!c) {
        delete e;
        return CMDG_ERR_INVALID;
    }
    c->eng = e;
    *out = c;
    return CMDG_OK;
}

int cmdg_create(const cmdg_desc *d, cmdg_handle *out)
{
    if (!d || !out) return CMDG_ERR_INVALID;
    if (d->dim == 3 && d->N[2] == 0) {
        *out = nullptr;
        g_create_err = "cmdg_create: N[2] == 0 is a finite-volume vertical: use cmdg_create_dgfv";
        return CMDG_ERR_INVALID;
    }
    if (d->physics_id == CMDG_PHYSICS_ESDG_DRY_ATMOS) {
        *out = nullptr;
        g_create_err = "cmdg_create: the DryAtmosModel of the entropy-stable discretisation has no DGModel passes: "
                       "use cmdg_create_esdg";
        return CMDG_ERR_INVALID;
    }
    return create_handle(d, nullptr, out);
}

// DGFVModel(balance_law, grid, fv_reconstruction, nf1, nf2, nfgrad; direction)  DGFVModel.jl:22-69
int cmdg_create_dgfv(const cmdg_desc *d, const cmdg_fv_desc *fv, cmdg_handle *out)
{
    if (!d || !fv || !out) return CMDG_ERR_INVALID;
    *out = nullptr;
    auto refuse = [&](int code, const char *msg) {
        g_create_err = msg;
        return code;
    };
    if (d->dim != 3 || d->N[2] != 0)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: the vertical polynomial order N[2] must be 0 (use cmdg_create otherwise)");
    if (!d->stacked)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: the finite-volume vertical needs a stacked grid");
    if (fv->nvertelem < 2)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: nvertelem < 2");
    const int recon = fv->reconstruction & ~CMDG_FV_HYDROSTATIC;
    if (recon != CMDG_FV_CONSTANT && recon != CMDG_FV_LINEAR)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: unknown reconstruction");
    if (fv->width < 0 || fv->width > 3)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: reconstruction width outside 0..3");
    if (recon == CMDG_FV_LINEAR && fv->width == 0)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: a linear reconstruction needs width >= 1");
    if (recon == CMDG_FV_CONSTANT && fv->width != 0)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: the constant reconstruction has width 0");
    if (fv->limiter != CMDG_FV_VANLEER && fv->limiter != CMDG_FV_NOLIMITER)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: unknown slope limiter");
    if (d->nreal % fv->nvertelem != 0 || d->nghost % fv->nvertelem != 0)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_dgfv: element counts are not multiples of nvertelem");
    return create_handle(d, fv, out);
}

// ESDGModel(balance_law, grid; volume_numerical_flux_first_order, surface_numerical_flux_first_order)
// ESDGModel.jl:75-94
int cmdg_create_esdg(const cmdg_desc *d, const cmdg_esdg_desc *ed, cmdg_handle *out)
{
    if (!d || !ed || !out) return CMDG_ERR_INVALID;
    *out = nullptr;
    auto refuse = [&](int code, const char *msg) {
        g_create_err = msg;
        return code;
    };
    if (d->physics_id != CMDG_PHYSICS_ESDG_DRY_ATMOS)
        return refuse(CMDG_ERR_UNSUPPORTED, "cmdg_create_esdg: the two-point fluxes are defined for CMDG_PHYSICS_ESDG_DRY_ATMOS only");
    if (d->dim != 3)
        return refuse(CMDG_ERR_UNSUPPORTED, "cmdg_create_esdg: only dim == 3 is compiled in");
    if (d->N[0] != d->N[1] || d->N[0] != d->N[2])
        return refuse(CMDG_ERR_UNSUPPORTED, "cmdg_create_esdg: mixed polynomial orders are not compiled in (one order in every direction)");
    if (d->N[0] != 3 && d->N[0] != 4)
        return refuse(CMDG_ERR_UNSUPPORTED, "cmdg_create_esdg: the flux-differencing kernel is compiled for polynomial orders 3 and 4");
    const int vf = ed->volume_flux, sf = ed->surface_flux;
    if (vf != CMDG_ESDG_FLUX_NONE && vf != CMDG_ESDG_FLUX_ENTROPY_CONSERVATIVE && vf != CMDG_ESDG_FLUX_CENTRAL &&
        vf != CMDG_ESDG_FLUX_KG)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_esdg: unknown volume flux");
    if (sf != CMDG_ESDG_FLUX_NONE && sf != CMDG_ESDG_FLUX_ENTROPY_CONSERVATIVE && sf != CMDG_ESDG_FLUX_RUSANOV &&
        sf != CMDG_ESDG_FLUX_ENTROPY_CONSERVATIVE_PENALTY && sf != CMDG_ESDG_FLUX_MATRIX)
        return refuse(CMDG_ERR_INVALID, "cmdg_create_esdg: unknown surface flux");
    cmdg_desc dd = *d;  // (nf_first, direction: not read by an ESDG handle)
    dd.nf_first = CMDG_RUSANOV;
    dd.direction = dd.diffusion_direction = CMDG_EVERY_DIRECTION;
    return create_handle(&dd, nullptr, out, ed);
}

// what a DGFVModel handle adds to init(): exchanges packed / unpacked as the reference does, and
// element lists that are whole stacks, bottom element first
int EngineBase::init_fv()
{
    reference_halo = true;
    const int nv = fv_nvert;
    // (fv.h fv_lds_bytes: primitives, face fluxes and cell weights of one stack; FV_LDS_MAX)
    if (sizeof(double) * NQ * NQ * ((size_t)ns * nv + (size_t)ns * (nv + 1) + nv) > 160 * 1024)
        return fail(CMDG_ERR_UNSUPPORTED, "cmdg_create_dgfv: a stack of this height does not fit the 160 KiB of LDS "
                                          "a work-group may own, in which the finite-volume pass stages it");
    if (const int r = fv_prepare()) return r;  // the law's say on the reconstruction; the LDS limit
    for (int which = 0; which < 2; ++which) {
        const int64_t n = which ? nexterior : ninterior;
        if (n == 0) continue;
        std::vector<int64_t> h((size_t)n);
        HIPCHK(hipMemcpy(h.data(), which ? d_exterior_user : d_interior_user, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
        bool ok = n % nv == 0;
        for (int64_t i = 0; ok && i < n; ++i)
            ok = h[i] >= 1 && h[i] <= nreal && (h[i] - 1) % nv == i % nv && (i % nv == 0 || h[i] == h[i - 1] + 1);
        if (!ok)
            return fail(CMDG_ERR_INVALID, "cmdg_create_dgfv: interiorelems / exteriorelems must list whole stacks, "
                                          "bottom element first");
    }
    return CMDG_OK;
}

int cmdg_destroy(cmdg_handle h)
{
    if (!h) return CMDG_ERR_INVALID;
    {
        DevGuard guard_(h->eng);
        // handles whose hooks evaluate this one as their nested operator cannot evaluate any more
        // (they would compute something else than the law they were given): their next evaluation
        // fails until cmdg_set_rhs_hooks gives them new hooks; the nested operator of this handle
        // forgets its parent
        for (EngineBase *parent : h->eng->nested_in) {
            parent->synchronize();
            parent->hooks.pre_rhs_handle = nullptr;
            parent->hooks_orphaned = true;
        }
        if (h->eng->has_hooks && h->eng->hooks.pre_rhs_handle && h->eng->hooks.pre_rhs_handle->eng) {
            auto &v = h->eng->hooks.pre_rhs_handle->eng->nested_in;
            v.erase(std::remove(v.begin(), v.end(), h->eng), v.end());
        }
        // members of a local group keep pointers to each other: detach the survivors
        for (EngineBase *peer : h->eng->group)
            if (peer && peer != h->eng) {
                peer->group.clear();
                peer->transport = TRANSPORT_NONE;
            }
        reduce_release(h->eng);
        les_release(h->eng);
        delete h->eng;
    }
    delete h;
    return CMDG_OK;
}

const char *cmdg_last_error(cmdg_handle h)
{
    if (!h) return g_create_err.c_str();
    return h->err.c_str();
}

}  // extern "C"
