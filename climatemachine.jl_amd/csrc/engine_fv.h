// Engine of a DGFVModel handle (cmdg_create_dgfv): spectral-element DG in the horizontal, a
// cell-centred finite volume method in the vertical.  The orchestration is EngineBase::rhs_segment
// unchanged -- (dgfvm::DGFVModel)(tendency, Q, _, t, alpha, beta) (DGFVModel.jl:85-320) cuts an
// evaluation at the same exchanges as the DGModel's -- with the two passes that have a vertical part
// launched as the reference launches them for a DGFVModel (SpaceDiscretization.jl:505,604,
// 1100-1158,1224-1278): the DG kernels at (NQ, NQV = 1) in the horizontal direction (faces 1-4,
// volume sources added), then the finite-volume kernel of fv.h on the same element list.  The
// vertical passes read their own stack only, so they need no halo of their own.
// The class sits on the law layer and names the DG kernels a DGFVModel handle launches: the gradient
// pass, and the one tendency variant with neither the fused update nor the receive buffers.  A law
// with hyperdiffusive states is refused at create, so its two passes are not compiled for it.
#pragma once
#include "engine.h"
#include "fv.h"

namespace cmdg {

template <class P, int NQ_>
struct EngineFV : EngineLaw<P, NQ_, 1> {
    using Base = EngineLaw<P, NQ_, 1>;
    cmdg_fv_desc fvd{};
    using FvKernel = void (*)(FvArgs<P>);

    FvArgs<P> fv_args(const RhsCtx &c, const int64_t *elems, int64_t n) const
    {
        FvArgs<P> a;
        a.prm = this->prm;
        a.g = this->g;
        a.elems = elems;
        a.nelems = n;
        a.nvert = fvd.nvertelem;
        a.Q = c.Qin;
        a.aux = this->aux;
        a.derived = this->derived;
        a.gf = this->gf;
        a.tendency = c.tendency;
        a.t = c.t;
        a.alpha = c.alpha;
        a.beta = c.beta;
        a.increment = this->direction == DIR_EVERY;
        a.add_source = this->direction == DIR_VERTICAL;
        a.model_dir = this->direction;
        a.nf_first = this->nf_first;
        a.recon = fvd.reconstruction & ~CMDG_FV_HYDROSTATIC;
        a.limiter = fvd.limiter;
        a.hydrostatic = (fvd.reconstruction & CMDG_FV_HYDROSTATIC) != 0;
        return a;
    }
    template <bool PERIODIC>
    static FvKernel pick_fv_tendency(int width)
    {
        switch (width) {
        case 0: return k_fv_tendency<P, NQ_, 0, PERIODIC>;
        case 1: return k_fv_tendency<P, NQ_, 1, PERIODIC>;
        case 2: return k_fv_tendency<P, NQ_, 2, PERIODIC>;
        default: return k_fv_tendency<P, NQ_, 3, PERIODIC>;
        }
    }
    FvKernel fv_tendency_kernel() const
    {
        return fvd.periodicstack ? pick_fv_tendency<true>(fvd.width) : pick_fv_tendency<false>(fvd.width);
    }
    // What create asks of the instantiation.  HBFVReconstruction needs a functor that names a
    // pressure primitive (law_defaults.h PRIM_P).  A stack whose staging passes the 64 KiB a launch
    // may ask for by default: the dynamic-LDS limit of the one tendency kernel this handle launches
    // is raised to what the stack needs (up to the 160 KiB a work-group may own on gfx950), on this
    // handle's device, when the handle is created.
    int fv_prepare() override
    {
        if ((fvd.reconstruction & CMDG_FV_HYDROSTATIC) && P::PRIM_P < 0)
            return this->fail(CMDG_ERR_INVALID, "cmdg_create_dgfv: CMDG_FV_HYDROSTATIC (HBFVReconstruction) needs a "
                                                "law that names a pressure primitive (the dry atmosphere law)");
        const size_t need = fv_lds_bytes(P::NS, NQ_ * NQ_, fvd.nvertelem);
        if (need <= FV_LDS_DEFAULT) return CMDG_OK;
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(fv_tendency_kernel()),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)need) != hipSuccess) {
            (void)hipGetLastError();
            return this->fail(CMDG_ERR_UNSUPPORTED, "cmdg_create_dgfv: the device refuses the LDS a stack of this "
                                                    "height is staged in");
        }
        return CMDG_OK;
    }
    int launch_gradients(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) override
    {
        if (n <= 0) return CMDG_OK;
        int r = CMDG_OK;
        if (this->diffusion_direction != DIR_VERTICAL) {
            r = this->in_pass(Base::GRADIENTS, n, exterior, st, [&] {
                const PassArgs<P> args = this->make_args(c, elems, n, DIR_HORIZONTAL, exterior, nullptr, nullptr);
                return this->launch_picked(gradients_kernel<P, NQ_, 1>(this->gf_live()), (unsigned)n, KDims<NQ_, 1>::NT,
                                           st, args, "gradient", "gf_live = %d", (int)this->gf_live());
            });
            if (r != CMDG_OK) return r;
        }
        if (this->diffusion_direction != DIR_HORIZONTAL && P::NGF > 0 && this->gf_live()) {
            this->prof_begin(CMDG_K_FV_GRADIENTS, st);
            FvArgs<P> a = fv_args(c, elems, n);
            // (SpaceDiscretization.jl:717-719: increments after the horizontal values of an
            // EveryDirection model)
            a.increment = this->direction == DIR_EVERY;
            const int64_t nthreads = n * NQ_ * NQ_;
            FvKernel k = k_fv_gradients<P, NQ_, false>;
            if (fvd.periodicstack) k = k_fv_gradients<P, NQ_, true>;
            hipLaunchKernelGGL(k, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, st, a);
            this->prof_end(st);
        }
        return CMDG_OK;
    }
    int launch_divgrad(const RhsCtx &, const int64_t *, int64_t, bool, hipStream_t) override
    {
        return this->no_pass("Laplacian", "DGFVModel");
    }
    int launch_gradlap(const RhsCtx &, const int64_t *, int64_t, bool, hipStream_t) override
    {
        return this->no_pass("gradient-of-Laplacian", "DGFVModel");
    }
    int launch_tendency(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) override
    {
        if (n <= 0) return CMDG_OK;
        if (this->direction != DIR_VERTICAL) {
            const int r = this->in_pass(Base::TENDENCY, n, exterior, st, [&] {
                using SH = TendencyShape<P, NQ_, 1>;
                const PassArgs<P> args = this->make_args(c, elems, n, DIR_HORIZONTAL, exterior, nullptr, nullptr);
                const bool gf = needs_gradflux<P>(this->prm);
                return this->launch_picked(tendency_kernel<P, NQ_, 1, false, false>(gf), (unsigned)SH::blocks(n),
                                           SH::NT, st, args, "tendency", "gradient flux = %d", (int)gf);
            });
            if (r != CMDG_OK) return r;
        }
        if (this->direction != DIR_HORIZONTAL) {
            this->prof_begin(CMDG_K_FV_TENDENCY, st);
            const FvArgs<P> a = fv_args(c, elems, n);
            const int nv = fvd.nvertelem;
            const FvKernel k = fv_tendency_kernel();
            hipLaunchKernelGGL(k, dim3((unsigned)(n / nv)), dim3(fv_threads(NQ_ * NQ_, nv)),
                               fv_lds_bytes(P::NS, NQ_ * NQ_, nv), st, a);
            this->prof_end(st);
        }
        return CMDG_OK;
    }
};

template <class P, int NQ_>
EngineBase *make_engine_fv(const cmdg_desc *d, const cmdg_fv_desc *fv)
{
    auto *e = new EngineFV<P, NQ_>();
    e->init_law(d);
    e->fv = true;
    e->fv_nvert = fv->nvertelem;
    e->fvd = *fv;
    return e;
}

}  // namespace cmdg
