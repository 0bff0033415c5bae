// libcmdg: host code of the column operators (stack integrals, the recorded hooks of
// update_auxiliary_state! / update_auxiliary_state_gradient!) and of the element filters.
#include <algorithm>
#include <memory>
#include <new>

#include "stepping.h"
#include "columns.h"
#include "filters.h"
#include "with_constant.h"

namespace cmdg {

// ---- the argument structs, filled in one place each ----------------------------------------------
// what every launch over the stacks [h0, h0 + nhorz) of a handle shares; the integrands are the caller's
static StackArgs stack_args(const EngineBase &e, const double *Q, int nstate, double *aux_arr, int naux_arr,
                            int nvert, int64_t h0, int64_t nhorz)
{
    StackArgs a{};
    a.Q = Q;
    a.aux = aux_arr;
    a.vgeo = e.g.vgeo;
    a.Imat = e.d_Imat;
    a.nstate = nstate;
    a.naux = naux_arr;
    a.nvgeo = e.g.nvgeo;
    a.nvert = nvert;
    a.jcv = JCV;
    a.h0 = h0;
    a.nhorz = nhorz;
    return a;
}

// what the launches of a filter on a state array of this handle share; the filtered states, the
// directions and the reference-state columns are the caller's
static FilterArgs filter_args(const EngineBase &e, const FilterObj *f, double *Q, int nstate)
{
    FilterArgs a{};
    a.Q = Q;
    a.aux = e.aux;
    a.vgeo = e.g.vgeo;
    a.Fh = f->d_Fh;
    a.Fv = f->d_Fv;
    a.nstate = nstate;
    a.naux = e.naux;
    a.nvgeo = e.g.nvgeo;
    a.nreal = e.nreal;
    return a;
}

// ---- indefinite_stack_integral! / reverse_indefinite_stack_integral!  DGModel.jl:445-529 ----
template <int NQ_, int NOUT>
static void launch_stack(bool reverse, const StackArgs &a, hipStream_t st)
{
    constexpr int SPB = 256 / (NQ_ * NQ_);
    const dim3 grid((unsigned)((a.nhorz + SPB - 1) / SPB)), block(256);
    if (reverse)
        hipLaunchKernelGGL((k_reverse_stack_integral<NQ_, NOUT>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_stack_integral<NQ_, NOUT>), grid, block, 0, st, a);
}

int EngineBase::stack_integral(bool reverse, const double *Q, int nstate, double *aux_arr,
                               int naux_arr, int nvert, const double *Imat_host,
                               const cmdg_stack_integral_desc *d, int64_t h0, int64_t nh)
{
    const char *const no_order = "stack integral: polynomial order not compiled in";
    if (esdg) return fail(CMDG_ERR_UNSUPPORTED, "stack integral: an ESDGModel handle serves no column operators");
    if (!column_orders()) return fail(CMDG_ERR_UNSUPPORTED, no_order);
    if (!stacked) return fail(CMDG_ERR_INVALID, "stack integral: the topology is not stacked");
    if (nvert < 1 || nreal % nvert != 0)
        return fail(CMDG_ERR_INVALID, "stack integral: nreal is not a multiple of nvertelem");
    if (d->nout < 1 || d->nout > CMDG_STACK_MAXOUT) return fail(CMDG_ERR_INVALID, "stack integral: nout");
    if (g.nvgeo <= JCV) return fail(CMDG_ERR_INVALID, "stack integral: vgeo lacks the JcV column");
    for (int s = 0; s < d->nout; ++s) {
        const bool st = !reverse && d->src_is_state[s] != 0;
        const int src = reverse ? d->rsrc_col[s] : d->src_col[s];
        const int dst = reverse ? d->rdst_col[s] : d->dst_col[s];
        if (st && !Q) return fail(CMDG_ERR_INVALID, "stack integral: state integrand without Q");
        if (src < 0 || src >= (st ? nstate : naux_arr) || dst < 0 || dst >= naux_arr)
            return fail(CMDG_ERR_INVALID, "stack integral: column out of range");
    }
    if (nh < 0) nh = nreal / nvert;
    if (nh == 0) return CMDG_OK;
    if (!reverse && Imat_host) {  // (NULL: the matrix uploaded by an earlier call / the hooks)
        if (!d_Imat) HIPCHK(d_Imat.alloc(NQ * NQ));
        HIPCHK(hipMemcpyAsync(d_Imat, Imat_host, sizeof(double) * NQ * NQ, hipMemcpyHostToDevice, s_comp));
        HIPCHK(hipStreamSynchronize(s_comp));  // Imat_host may be a temporary of the caller
    }
    if (!reverse && !d_Imat) return fail(CMDG_ERR_INVALID, "stack integral: Imat is NULL");
    StackArgs a = stack_args(*this, Q, nstate, aux_arr, naux_arr, nvert, h0, nh);
    // integrals of different variables are independent: four ride in one launch
    for (int c0 = 0; c0 < d->nout; c0 += 4) {
        const int n = std::min(4, d->nout - c0);
        for (int s = 0; s < n; ++s) {
            a.is_state[s] = reverse ? 0 : d->src_is_state[c0 + s];
            a.src[s] = reverse ? d->rsrc_col[c0 + s] : d->src_col[c0 + s];
            a.dst[s] = reverse ? d->rdst_col[c0 + s] : d->dst_col[c0 + s];
            a.scale[s] = d->scale[c0 + s];
        }
        prof_begin(CMDG_K_STACK_INTEGRAL, s_comp);
        const bool launched = with_constant<2, 8>(NQ, [&](auto nq) {
            with_constant<1, 4>(n, [&](auto nout) { launch_stack<nq(), nout()>(reverse, a, s_comp); });
        });
        prof_end(s_comp);
        if (!launched) return fail(CMDG_ERR_UNSUPPORTED, no_order);
    }
    return launch_status("stack integral launch");
}

// ---- law-specific update_auxiliary_state! / update_auxiliary_state_gradient! as hooks ----
int EngineBase::set_hooks(const cmdg_rhs_hooks *hk)
{
    auto forget_child = [&]() {  // this handle no longer evaluates its former nested operator
        if (has_hooks && hooks.pre_rhs_handle && hooks.pre_rhs_handle->eng) {
            auto &v = hooks.pre_rhs_handle->eng->nested_in;
            v.erase(std::remove(v.begin(), v.end(), this), v.end());
        }
    };
    if (hk && esdg)
        return fail(CMDG_ERR_UNSUPPORTED, "rhs hooks: an ESDGModel handle runs no update_auxiliary_state! composition");
    if (!hk) {
        forget_child();
        has_hooks = false;
        hooks_orphaned = false;
        hooks.pre_rhs_handle = nullptr;
        return CMDG_OK;
    }
    if (hk->npre < 0 || hk->npre > CMDG_MAX_HOOK_OPS || hk->ncopy < 0 || hk->ncopy > CMDG_MAX_HOOK_OPS ||
        hk->nsurf < 0 || hk->nsurf > CMDG_MAX_HOOK_OPS)
        return fail(CMDG_ERR_INVALID, "hooks: too many operations");
    if (gf_node_major() && hk->ncopy > 0)
        return fail(CMDG_ERR_UNSUPPORTED, "hooks: gradient-flux copies are not built for laws whose state_gradient_flux "
                                          "is node-major inside the library (the dry atmosphere)");
    const bool cols = hk->has_integral || hk->has_reverse_integral || hk->nsurf > 0 ||
                      hk->has_flow_deviation;
    if (cols && (!stacked || hk->nvertelem < 1 || nreal % hk->nvertelem || nghost % hk->nvertelem))
        return fail(CMDG_ERR_INVALID, "hooks: column operators need a stacked topology and nvertelem");
    for (int i = 0; i < hk->ncopy; ++i)
        if (hk->copy_gf_col[i] < 0 || hk->copy_gf_col[i] >= ngf || hk->copy_aux_col[i] < 0 ||
            hk->copy_aux_col[i] >= naux)
            return fail(CMDG_ERR_INVALID, "hooks: copy column out of range");
    for (int i = 0; i < hk->nsurf; ++i)
        if (hk->surf_src_col[i] < 0 || hk->surf_src_col[i] >= naux || hk->surf_dst_col[i] < 0 ||
            hk->surf_dst_col[i] >= naux || hk->surf_src_col[i] == hk->surf_dst_col[i])
            return fail(CMDG_ERR_INVALID, "hooks: surface column out of range (or source == destination)");
    for (int i = 0; i < hk->npre; ++i)
        if (!hk->pre_filter[i]) return fail(CMDG_ERR_INVALID, "hooks: NULL filter");
    if (hk->has_flow_deviation) {
        if (hk->flow_u_col < 0 || hk->flow_u_col + 2 > ns || hk->flow_ud_col < 0 ||
            hk->flow_ud_col + 2 > naux || !(hk->flow_H > 0))
            return fail(CMDG_ERR_INVALID, "hooks: flow deviation columns / depth");
        if (!d_flowint) HIPCHK(d_flowint.alloc((size_t)2 * Np * nelem));
    }
    if (hk->pre_rhs_handle) {
        EngineBase *ch = hk->pre_rhs_handle->eng;
        if (!ch || ch == this || ch->Np != Np || ch->nelem != nelem || ch->ns != ns || ch->dev != dev)
            return fail(CMDG_ERR_INVALID, "hooks: the nested operator must share grid, state and device");
        if (ch->nabrtorank != nabrtorank || ch->nreal != nreal)
            return fail(CMDG_ERR_INVALID, "hooks: the nested operator must live on the same partition (same neighbours)");
        if (hk->pre_rhs_src_col < 0 || hk->pre_rhs_src_col >= ch->ns || hk->pre_rhs_dst_aux_col < 0 ||
            hk->pre_rhs_dst_aux_col >= naux)
            return fail(CMDG_ERR_INVALID, "hooks: nested operator column out of range");
        if (!d_preT) HIPCHK(d_preT.alloc((size_t)Np * ch->ns * nelem));
    }
    if (hk->has_integral || hk->has_flow_deviation) {
        if (!hk->Imat) return fail(CMDG_ERR_INVALID, "hooks: Imat is NULL");
        if (!d_Imat) HIPCHK(d_Imat.alloc(NQ * NQ));
        HIPCHK(hipMemcpy(d_Imat, hk->Imat, sizeof(double) * NQ * NQ, hipMemcpyHostToDevice));
    }
    forget_child();
    hooks = *hk;
    hooks.Imat = nullptr;
    has_hooks = true;
    hooks_orphaned = false;
    if (hooks.pre_rhs_handle) hooks.pre_rhs_handle->eng->nested_in.push_back(this);
    return CMDG_OK;
}

// update_auxiliary_state!(dg, law, Q, t, realelems) as the recorded composition.  First half: the
// pre filters, and the context of the nested operator's evaluation (whose stream is made to follow
// this one); second half: its tendency column into the auxiliary state, the column operators, the
// flow deviation.  Between the two the nested operator is evaluated -- by run_pre_hooks itself for
// a single handle (one rank, or one RCCL rank per process: the nested operator exchanges with its
// own communicator, in the same order on every rank), by group_rhs in lock step for a local group.
int EngineBase::run_pre_hooks_a(const RhsCtx &c, RhsCtx &cc)
{
    if (hooks_orphaned)
        return fail(CMDG_ERR_INVALID, "hooks: the nested operator of this handle was destroyed; set new hooks");
    if (!filter_pair(c.Qin))  // (two vertical filters on disjoint states: one launch)
        for (int i = 0; i < hooks.npre; ++i)
            if (int r = filter_apply(reinterpret_cast<const FilterObj *>(hooks.pre_filter[i]), c.Qin, ns))
                return r;
    if (hooks.pre_rhs_handle) {
        // conti3d_dg(ct3d_dQ, Q, p, t; increment = false); A.w = dQ.theta  (OceanModel.jl:456-477)
        EngineBase *ch = hooks.pre_rhs_handle->eng;
        HIPCHK(ev_record(ev_comp, s_comp));
        HIPCHK(hipStreamWaitEvent(ch->s_comp, ev_comp, 0));
        cc = RhsCtx();
        cc.tendency = d_preT;
        cc.Qin = c.Qin;
        cc.t = c.t;
        cc.alpha = 1.0;
        cc.beta = 0.0;
    }
    return CMDG_OK;
}

// The two pre filters of the ocean models as one launch (filters.h k_apply_vfilter_pair) when they
// are vertical spectral FilterIndices filters on disjoint states; false: apply them one by one.
bool EngineBase::filter_pair(double *Q)
{
    if (fused_columns < 2 || hooks.npre != 2 || !column_orders() || nreal <= 0) return false;
    const FilterObj *f1 = reinterpret_cast<const FilterObj *>(hooks.pre_filter[0]);
    const FilterObj *f2 = reinterpret_cast<const FilterObj *>(hooks.pre_filter[1]);
    for (const FilterObj *f : {f1, f2})
        if (f->kind != CMDG_FILTER_SPECTRAL || f->target != CMDG_TARGET_INDICES || f->direction != DIR_VERTICAL)
            return false;
    if (f1->nindices + f2->nindices > 8) return false;
    for (int i = 0; i < f1->nindices; ++i) {
        if (f1->indices[i] > ns) return false;
        for (int j = 0; j < f2->nindices; ++j)
            if (f2->indices[j] > ns || f1->indices[i] == f2->indices[j]) return false;
    }
    FilterArgs a = filter_args(*this, f1, Q, ns);
    a.nfs = f1->nindices + f2->nindices;
    for (int i = 0; i < f1->nindices; ++i) a.idx[i] = f1->indices[i];
    for (int j = 0; j < f2->nindices; ++j) a.idx[f1->nindices + j] = f2->indices[j];
    a.do_h = 0, a.do_v = 1;
    prof_begin(CMDG_K_FILTER, s_comp);
    const bool launched = with_constant<2, 8>(NQ, [&](auto nq) {
        constexpr int N = nq();
        hipLaunchKernelGGL((k_apply_vfilter_pair<N>), dim3((unsigned)(((int64_t)N * N * a.nfs * nreal + 255) / 256)),
                           dim3(256), 0, s_comp, a, (const double *)f2->d_Fv, f1->nindices);
    });
    prof_end(s_comp);
    return launched;  // (column_orders(): always)
}

int EngineBase::run_pre_hooks_b(const RhsCtx &c)
{
    if (hooks.pre_rhs_handle) {
        EngineBase *ch = hooks.pre_rhs_handle->eng;
        HIPCHK(ev_record(ch->ev_comp, ch->s_comp));
        HIPCHK(hipStreamWaitEvent(s_comp, ch->ev_comp, 0));
        const int64_t n = nreal * Np;
        hipLaunchKernelGGL(k_scaled_column_copy, dim3(nblocks(n)), dim3(256), 0, s_comp, aux, naux,
                           hooks.pre_rhs_dst_aux_col, (const double *)d_preT, ch->ns, hooks.pre_rhs_src_col,
                           1.0, Np, (int64_t)0, nreal);
    }
    if (hooks.ops_before_gradients)
        if (int r = run_column_ops(c, 0, nreal)) return r;
    if (hooks.has_flow_deviation)
        if (int r = flow_deviation(c.Qin, 0, nreal / hooks.nvertelem)) return r;
    return CMDG_OK;
}

int EngineBase::run_pre_hooks(const RhsCtx &c)
{
    RhsCtx cc;
    if (int r = run_pre_hooks_a(c, cc)) return r;
    if (hooks.pre_rhs_handle) {
        EngineBase *ch = hooks.pre_rhs_handle->eng;
        if (int r = ch->rhs_async(cc)) return fail(r, "nested operator: " + ch->err);
    }
    return run_pre_hooks_b(c);
}

// compute_flow_deviation!(dg, ::HBModel, ::Coupled, Q, t)
// (HydrostaticBoussinesqCoupling.jl:43-85): u_d = u - (1/H) int u dz on the stacks
// [h0, h0 + nh).  For ghost stacks (after the exchange of Q) the integral runs over the received
// face pencils, which is all the neighbours read.
int EngineBase::flow_deviation(double *Q, int64_t h0, int64_t nh)
{
    if (nh <= 0) return CMDG_OK;
    if (fused_columns && column_orders() && g.nvgeo > JCV && d_Imat) {
        // integral and subtraction in one launch (columns.h k_flow_deviation)
        prof_begin(CMDG_K_STACK_INTEGRAL, s_comp);
        const bool launched = with_constant<2, 8>(NQ, [&](auto nq) {
            constexpr int N = nq(), SPB = 256 / (N * N);
            hipLaunchKernelGGL((k_flow_deviation<N>), dim3((unsigned)((nh + SPB - 1) / SPB)), dim3(256), 0, s_comp,
                               (const double *)Q, ns, hooks.flow_u_col, aux, naux, hooks.flow_ud_col, g.vgeo, g.nvgeo,
                               JCV, (const double *)d_Imat, hooks.flow_H, hooks.nvertelem, h0, nh);
        });
        prof_end(s_comp);
        return launched ? CMDG_OK : fail(CMDG_ERR_UNSUPPORTED, "flow deviation: polynomial order not compiled in");
    }
    if (int r = integrate_velocity(Q, ns, hooks.flow_u_col, hooks.nvertelem, h0, nh)) return r;
    const int64_t n = nh * hooks.nvertelem * Np;
    hipLaunchKernelGGL(k_column_minus_top_over_H, dim3(nblocks(n)), dim3(256), 0, s_comp, aux, naux,
                       hooks.flow_ud_col, (const double *)Q, ns, hooks.flow_u_col, (const double *)d_flowint,
                       hooks.flow_H, NQ * NQ, NQ, hooks.nvertelem, h0, nh);
    return CMDG_OK;
}

// update_auxiliary_state!(integral_model, ...) of VerticalIntegralModel.jl:60-81: the upward
// column integral of X[:, col..col+1, :] into the scratch d_flowint (Np, 2, nelem)
int EngineBase::integrate_velocity(const double *X, int nstate, int col, int nvert, int64_t h0,
                                   int64_t nh)
{
    if (nh < 0) nh = nreal / nvert;
    if (!d_flowint) HIPCHK(d_flowint.alloc((size_t)2 * Np * nelem));
    cmdg_stack_integral_desc d{};
    d.nout = 2;
    for (int c = 0; c < 2; ++c) {
        d.src_is_state[c] = 1;
        d.src_col[c] = col + c;
        d.scale[c] = 1.0;
        d.dst_col[c] = c;
    }
    return stack_integral(false, X, nstate, d_flowint, 2, nvert, nullptr, &d, h0, nh);
}

int EngineBase::run_gradient_hooks(const RhsCtx &c, int64_t e0, int64_t e1)
{
    if (e1 <= e0) return CMDG_OK;
    if (!hooks.ops_before_gradients && column_chain(c, e0, e1, true)) return CMDG_OK;
    const int64_t n = (e1 - e0) * Np;
    const unsigned nb = nblocks(n);
    for (int i = 0; i < hooks.ncopy; ++i)
        hipLaunchKernelGGL(k_scaled_column_copy, dim3(nb), dim3(256), 0, s_comp, aux, naux,
                           hooks.copy_aux_col[i], gf, ngf, hooks.copy_gf_col[i], hooks.copy_scale[i],
                           Np, e0, e1);
    if (hooks.ops_before_gradients) return CMDG_OK;  // done in update_auxiliary_state! already
    return run_column_ops(c, e0, e1);
}

// The recorded composition copy -> upward integrals -> reverse integral -> surface value as ONE
// launch (columns.h k_column_chain) when it has the shape the ocean models record: every copied
// gradient-flux column is the integrand AND the destination of one upward integral, every
// reverse integral runs in place on an upward integral's result, every surface value is taken from
// an upward integral that is not reversed.  Anything else: false, and the caller issues the
// operations one by one.
bool EngineBase::column_chain(const RhsCtx &c, int64_t e0, int64_t e1, bool with_copies)
{
    if (!fused_columns || !hooks.has_integral || !column_orders() || g.nvgeo <= JCV || !d_Imat) return false;
    const cmdg_stack_integral_desc &d = hooks.integral;
    const int nv = hooks.nvertelem;
    if (d.nout < 1 || d.nout > 4 || !stacked || nv < 1) return false;
    ChainArgs ch{};
    StackArgs &a = ch.a;
    a = stack_args(*this, c.Qin, ns, aux, naux, nv, e0 / nv, (e1 - e0) / nv);
    ch.gf = gf;
    ch.ngf = ngf;
    for (int s = 0; s < STACK_MAXOUT; ++s) ch.gf_col[s] = ch.rev_dst[s] = ch.surf_dst[s] = -1;
    for (int s = 0; s < d.nout; ++s) {
        a.is_state[s] = d.src_is_state[s];
        a.src[s] = d.src_col[s];
        a.dst[s] = d.dst_col[s];
        a.scale[s] = d.scale[s];
        if (d.src_is_state[s] && !c.Qin) return false;
    }
    if (with_copies)
        for (int i = 0; i < hooks.ncopy; ++i) {
            int hit = -1;
            for (int s = 0; s < d.nout; ++s)
                if (!d.src_is_state[s] && d.src_col[s] == hooks.copy_aux_col[i] &&
                    d.dst_col[s] == hooks.copy_aux_col[i] && ch.gf_col[s] < 0)
                    hit = s;
            // the copied column must feed exactly that integral (nobody else reads the copy)
            for (int s = 0; s < d.nout; ++s)
                if (s != hit && !d.src_is_state[s] && d.src_col[s] == hooks.copy_aux_col[i]) hit = -1;
            if (hit < 0) return false;
            ch.gf_col[hit] = hooks.copy_gf_col[i];
            ch.gf_scale[hit] = hooks.copy_scale[i];
        }
    if (hooks.has_reverse_integral) {
        const cmdg_stack_integral_desc &r = hooks.reverse_integral;
        for (int q = 0; q < r.nout; ++q) {
            int hit = -1;
            for (int s = 0; s < d.nout; ++s)
                if (d.dst_col[s] == r.rsrc_col[q] && r.rdst_col[q] == r.rsrc_col[q] && ch.rev_dst[s] < 0) hit = s;
            if (hit < 0) return false;
            ch.rev_dst[hit] = r.rdst_col[q];
        }
    }
    for (int i = 0; i < hooks.nsurf; ++i) {
        int hit = -1;
        for (int s = 0; s < d.nout; ++s)
            if (d.dst_col[s] == hooks.surf_src_col[i] && ch.rev_dst[s] < 0 && ch.surf_dst[s] < 0) hit = s;
        if (hit < 0) return false;
        for (int s = 0; s < d.nout; ++s)  // the destination is nobody's integrand or result
            if (hooks.surf_dst_col[i] == d.dst_col[s] || (!d.src_is_state[s] && hooks.surf_dst_col[i] == d.src_col[s]))
                return false;
        ch.surf_dst[hit] = hooks.surf_dst_col[i];
    }
    // (two upward integrals must not write one column, nor read what another one writes)
    for (int s = 0; s < d.nout; ++s)
        for (int q = 0; q < d.nout; ++q)
            if (q != s && (d.dst_col[s] == d.dst_col[q] || (!d.src_is_state[q] && d.src_col[q] == d.dst_col[s])))
                return false;
    if (a.nhorz <= 0) return true;
    prof_begin(CMDG_K_STACK_INTEGRAL, s_comp);
    const bool launched = with_constant<2, 8>(NQ, [&](auto nq) {
        constexpr int N = nq(), SPB = 256 / (N * N);
        const dim3 grid((unsigned)((a.nhorz + SPB - 1) / SPB)), block(256);
        with_constant<1, 4>(d.nout, [&](auto nout) {
            hipLaunchKernelGGL((k_column_chain<N, nout()>), grid, block, 0, s_comp, ch);
        });
    });
    prof_end(s_comp);
    return launched;  // (column_orders() and 1 <= nout <= 4: always)
}

// upward integral, downward integral, surface value down the column: elements [e0, e1)
int EngineBase::run_column_ops(const RhsCtx &c, int64_t e0, int64_t e1)
{
    if (e1 <= e0) return CMDG_OK;
    if (column_chain(c, e0, e1, false)) return CMDG_OK;
    const int64_t n = (e1 - e0) * Np;
    const unsigned nb = nblocks(n);
    const int nv = hooks.nvertelem;
    if (hooks.has_integral)
        if (int r = stack_integral(false, c.Qin, ns, aux, naux, nv, nullptr, &hooks.integral, e0 / nv,
                                   (e1 - e0) / nv))
            return r;
    if (hooks.has_reverse_integral)
        if (int r = stack_integral(true, nullptr, 0, aux, naux, nv, nullptr, &hooks.reverse_integral,
                                   e0 / nv, (e1 - e0) / nv))
            return r;
    for (int i = 0; i < hooks.nsurf; ++i)
        hipLaunchKernelGGL(k_surface_to_column, dim3(nb), dim3(256), 0, s_comp, aux, naux,
                           hooks.surf_src_col[i], hooks.surf_dst_col[i], NQ * NQ, NQ, nv, e0 / nv,
                           (e1 - e0) / nv);
    return CMDG_OK;
}

// ---- Filters.apply_async!   Filters.jl:440-607 ----------------------------------------
int EngineBase::filter_create(const cmdg_filter_desc *d, FilterObj **out)
{
    if (fv) return fail(CMDG_ERR_UNSUPPORTED, "filter: element filters are not defined on a DGFVModel handle (vertical order 0)");
    if (esdg) return fail(CMDG_ERR_UNSUPPORTED, "filter: an ESDGModel handle applies no element filters");
    if (d->kind < CMDG_FILTER_SPECTRAL || d->kind > CMDG_FILTER_TMAR)
        return fail(CMDG_ERR_INVALID, "filter: unknown kind");
    if (d->target < CMDG_TARGET_INDICES || d->target > CMDG_TARGET_ATMOS_SPECIFIC_PERTURBATIONS)
        return fail(CMDG_ERR_INVALID, "filter: unknown target");
    if (d->direction < 0 || d->direction > 2) return fail(CMDG_ERR_INVALID, "filter: bad direction");
    if (d->kind == CMDG_FILTER_TMAR && d->target != CMDG_TARGET_INDICES)
        return fail(CMDG_ERR_INVALID, "TMAR filter takes FilterIndices targets");
    if (d->target == CMDG_TARGET_INDICES) {
        if (d->nindices < 1 || d->nindices > CMDG_MAX_FILTER_STATES)
            return fail(CMDG_ERR_INVALID, "filter: 1..32 filtered states");
        for (int i = 0; i < d->nindices; ++i)
            if (d->indices[i] < 1) return fail(CMDG_ERR_INVALID, "filter: indices are 1-based");
    } else if (d->aux_ref_rho < 0 || d->aux_ref_rho >= naux || d->aux_ref_rhoe < 0 ||
               d->aux_ref_rhoe >= naux) {
        return fail(CMDG_ERR_INVALID, "filter: reference-state columns outside state_auxiliary");
    }
    if (d->kind != CMDG_FILTER_TMAR && (!d->filter_h || !d->filter_v))
        return fail(CMDG_ERR_INVALID, "filter: filter matrices are NULL");
    std::unique_ptr<FilterObj> f(new (std::nothrow) FilterObj());
    if (!f) return fail(CMDG_ERR_INVALID, "filter: out of memory");
    f->kind = d->kind;
    f->target = d->target;
    f->direction = d->direction;
    f->nindices = d->nindices;
    for (int i = 0; i < CMDG_MAX_FILTER_STATES; ++i) f->indices[i] = d->indices[i];
    f->aux_ref_rho = d->aux_ref_rho;
    f->aux_ref_rhoe = d->aux_ref_rhoe;
    if (d->kind != CMDG_FILTER_TMAR) {
        const size_t nb = sizeof(double) * NQ * NQ;
        if (f->d_Fh.alloc(NQ * NQ) != hipSuccess || f->d_Fv.alloc(NQ * NQ) != hipSuccess ||
            hipMemcpy(f->d_Fh, d->filter_h, nb, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(f->d_Fv, d->filter_v, nb, hipMemcpyHostToDevice) != hipSuccess)
            return fail(CMDG_ERR_HIP, "filter: upload of the filter matrices failed");
    }
    *out = f.release();
    return CMDG_OK;
}

static_assert(FILTER_FAM_SPECTRAL == CMDG_FILTER_SPECTRAL && FILTER_FAM_MASS_PRESERVING == CMDG_FILTER_MASS_PRESERVING &&
                  FILTER_FAM_TMAR == CMDG_FILTER_TMAR,
              "filter_lds.h numbers the kernel families as cmdg.h numbers the filter kinds");

template <int NQ_>
static void launch_filter(const FilterObj *f, const FilterArgs &a, int nfs, int64_t nreal,
                          hipStream_t st)
{
    const dim3 grid((unsigned)nreal), block(FDims<NQ_>::NT);
    const size_t lds = sizeof(double) * filter_dynamic_doubles(f->kind, NQ_, nfs);
    auto spectral = [&](auto K) { hipLaunchKernelGGL(K, grid, block, lds, st, a); };
    if (f->kind == CMDG_FILTER_TMAR) {
        hipLaunchKernelGGL((k_apply_tmar_filter<NQ_>), grid, dim3(64), 0, st, a);
    } else if (f->kind == CMDG_FILTER_SPECTRAL) {
        if (f->target == CMDG_TARGET_INDICES) spectral(k_apply_filter<NQ_, TGT_INDICES>);
        else if (f->target == CMDG_TARGET_ATMOS_PERTURBATIONS) spectral(k_apply_filter<NQ_, TGT_ATMOS_PERT>);
        else spectral(k_apply_filter<NQ_, TGT_ATMOS_SPECIFIC>);
    } else {
        if (f->target == CMDG_TARGET_INDICES) spectral(k_apply_mp_filter<NQ_, TGT_INDICES>);
        else if (f->target == CMDG_TARGET_ATMOS_PERTURBATIONS) spectral(k_apply_mp_filter<NQ_, TGT_ATMOS_PERT>);
        else spectral(k_apply_mp_filter<NQ_, TGT_ATMOS_SPECIFIC>);
    }
}

int EngineBase::filter_apply(const FilterObj *f, double *Q, int nstate)
{
    if (!f || !Q) return fail(CMDG_ERR_INVALID, "filter: NULL argument");
    const char *const no_order = "filter: polynomial order not compiled in";
    if (!column_orders()) return fail(CMDG_ERR_UNSUPPORTED, no_order);
    if (nreal <= 0) return CMDG_OK;
    FilterArgs a = filter_args(*this, f, Q, nstate);
    a.aux_rho = f->aux_ref_rho;
    a.aux_rhoe = f->aux_ref_rhoe;
    bool launched = true;
    auto launch = [&] {
        launched &= with_constant<2, 8>(NQ, [&](auto nq) { launch_filter<nq()>(f, a, a.nfs, nreal, s_comp); });
    };
    if (f->target == CMDG_TARGET_INDICES) {
        for (int i = 0; i < f->nindices; ++i)
            if (f->indices[i] > nstate) return fail(CMDG_ERR_INVALID, "filter: index beyond nstate");
    } else if (nstate != ATMOS_NS) {
        return fail(CMDG_ERR_INVALID, "filter: atmos targets need the 5-variable dry state");
    }
    const bool every = f->direction == DIR_EVERY;
    const bool h = every || f->direction == DIR_HORIZONTAL, v = every || f->direction == DIR_VERTICAL;
    // FilterIndices states are independent: at most CHUNK of them share the LDS of a launch, the most
    // whose buffers, with the kernel family's static arrays, stay within 64 KiB (filter_lds.h)
    const int CHUNK = filter_chunk(f->kind, NQ);
    const int ntot = f->target == CMDG_TARGET_INDICES ? f->nindices : ATMOS_NS;
    if (CHUNK < (f->target == CMDG_TARGET_INDICES ? 1 : ATMOS_NS)) return fail(CMDG_ERR_UNSUPPORTED, no_order);
    for (int c0 = 0; c0 < ntot; c0 += CHUNK) {
        const int nfs = std::min(CHUNK, ntot - c0);
        a.nfs = nfs;
        for (int i = 0; i < nfs; ++i) a.idx[i] = f->indices[c0 + i];
        prof_begin(CMDG_K_FILTER, s_comp);
        if (f->kind == CMDG_FILTER_MASS_PRESERVING) {
            // one launch per direction, each with its own mass correction (Filters.jl:566-605)
            if (h) {
                a.do_h = 1, a.do_v = 0;
                launch();
            }
            if (v) {
                a.do_h = 0, a.do_v = 1;
                launch();
            }
        } else {
            a.do_h = h, a.do_v = v;
            launch();
        }
        prof_end(s_comp);
    }
    if (!launched) return fail(CMDG_ERR_UNSUPPORTED, no_order);
    return launch_status("filter launch");
}

}  // namespace cmdg

using namespace cmdg;

extern "C" {

int cmdg_indefinite_stack_integral(cmdg_handle h, const double *Q, int32_t nstate, double *aux,
                                   int32_t naux, int32_t nvertelem, const double *Imat,
                                   const cmdg_stack_integral_desc *d)
{
    if (!h || !aux || !d || naux < 1) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->stack_integral(false, Q, nstate, aux, naux, nvertelem, Imat, d));
}

int cmdg_reverse_indefinite_stack_integral(cmdg_handle h, double *aux, int32_t naux,
                                           int32_t nvertelem, const cmdg_stack_integral_desc *d)
{
    if (!h || !aux || !d || naux < 1) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->stack_integral(true, nullptr, 0, aux, naux, nvertelem, nullptr, d));
}

int cmdg_filter_create(cmdg_handle h, const cmdg_filter_desc *d, cmdg_filter *out)
{
    if (!h || !d || !out) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    FilterObj *f = nullptr;
    int r = h->eng->filter_create(d, &f);
    *out = reinterpret_cast<cmdg_filter>(f);
    return set_err(h, r);
}

int cmdg_filter_destroy(cmdg_handle h, cmdg_filter f)
{
    if (!h || !f) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    FilterObj *o = reinterpret_cast<FilterObj *>(f);
    e->synchronize();
    if (e->gradient_filter == o) e->gradient_filter = nullptr;
    if (e->tendency_filter == o) e->tendency_filter = nullptr;
    if (e->step_filter == o) e->step_filter = nullptr;
    // a recorded update_auxiliary_state! composition may name this filter: drop it from there
    {
        int k = 0;
        for (int i = 0; i < e->hooks.npre; ++i)
            if (e->hooks.pre_filter[i] != f) e->hooks.pre_filter[k++] = e->hooks.pre_filter[i];
        e->hooks.npre = k;
    }
    delete o;
    return CMDG_OK;
}

int cmdg_filter_apply(cmdg_handle h, cmdg_filter f, double *Q, int32_t nstate)
{
    if (!h || !f || !Q || nstate < 1) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    return set_err(h, h->eng->filter_apply(reinterpret_cast<FilterObj *>(f), Q, nstate));
}

int cmdg_set_filters(cmdg_handle h, cmdg_filter gradient_filter, cmdg_filter tendency_filter,
                     cmdg_filter step_filter)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    EngineBase *e = h->eng;
    auto *gfl = reinterpret_cast<FilterObj *>(gradient_filter);
    auto *tfl = reinterpret_cast<FilterObj *>(tendency_filter);
    for (FilterObj *o : {gfl, tfl})
        if (o && o->target != CMDG_TARGET_INDICES)
            return set_err(h, e->fail(CMDG_ERR_INVALID, "gradient/tendency filters take FilterIndices targets"));
    // filters decide which streams the next evaluation's launches go to: start it from a clean slate
    if (int r = e->synchronize()) return set_err(h, r);
    e->invalidate_sends();
    e->drop_graph();
    e->gradient_filter = gfl;
    e->tendency_filter = tfl;
    e->step_filter = reinterpret_cast<FilterObj *>(step_filter);
    return CMDG_OK;
}

int cmdg_set_rhs_hooks(cmdg_handle h, const cmdg_rhs_hooks *hooks)
{
    if (!h) return CMDG_ERR_INVALID;
    DevGuard guard_(h->eng);
    if (int r = h->eng->synchronize()) return set_err(h, r);  // (hooks change the stream layout too)
    h->eng->invalidate_sends();
    h->eng->drop_graph();
    return set_err(h, h->eng->set_hooks(hooks));
}

}  // extern "C"
