// The template layer of the engine: EngineT<P, NQ, NQV> launches the pass kernels (kernels.h) of one
// balance law at one polynomial order for the host engine of engine_base.h, on top of the law layer of
// engine_law.h.  The engine_*.hip units and the generated plug-ins (plugins.py) include this header;
// everything else includes engine_base.h.
#pragma once
#include "engine_law.h"
#include "kernels.h"

namespace cmdg {

// The gradient and tendency kernels by what the law can ask of its gradient flux (law_defaults.h
// GRADFLUX): the USE_GF value a law rules out is not named for it, and asking for it gives null.
// state_gradient_flux is formed (EngineBase::gf_live) only by a law that has the states -- for any of
// them CMDG_OPT_KEEP_GRADFLUX may ask -- and is always formed for a law that always reads it.
template <class P, int NQ, int NQV>
PassKernel<P> gradients_kernel(bool gf_live)
{
    if constexpr (P::NGF > 0)
        if (gf_live) return k_gradients<P, NQ, NQV, true>;
    // (without the gradient flux the pass runs for the hyperdiffusion alone: rhs_segment's `grad`)
    if constexpr (gradflux_of<P> != GradFlux::always && P::NHYP > 0)
        if (!gf_live) return k_gradients<P, NQ, NQV, false>;
    return nullptr;
}
template <class P, int NQ, int NQV, bool LSRK, bool RECV>
PassKernel<P> tendency_kernel(bool gf)
{
    if constexpr (gradflux_of<P> != GradFlux::never)
        if (gf) return k_tendency<P, NQ, NQV, LSRK, true, RECV>;
    if constexpr (gradflux_of<P> != GradFlux::always)
        if (!gf) return k_tendency<P, NQ, NQV, LSRK, false, RECV>;
    return nullptr;
}

// ---------------------------------------------------------------------------------
template <class P, int NQ_, int NQV_ = NQ_>
struct EngineT : EngineLaw<P, NQ_, NQV_> {
    using Law = EngineLaw<P, NQ_, NQV_>;
    using Kernel = typename Law::Kernel;
    using Law::HO, Law::ELIDE, Law::make_args, Law::in_pass, Law::launch_picked, Law::prm;
    using Law::GRADIENTS, Law::DIVGRAD, Law::GRADLAP, Law::TENDENCY;
    using Law::slot, Law::g, Law::gf_live, Law::ngl, Law::direction, Law::diffusion_direction;
    using Law::d_lapI, Law::d_lapT;
    // ---- the four passes ---------------------------------------------------------------------
    // The instantiation of a pass kernel for the flags of a launch.  A combination the law does not
    // instantiate (GradArgHandoff, GRADFLUX) is not named for it; the flags never ask for one
    // (handoff_eligible, needs_gradflux), and a launcher that is handed null fails the evaluation.
    static Kernel pick_gradients(bool gf_live, bool garg_in)
    {
        if (garg_in) {
            if constexpr (HO)  // (handoff_eligible: no gradient flux, no ghosts)
                return k_gradients<P, NQ_, NQV_, false, true>;
            return nullptr;
        }
        return gradients_kernel<P, NQ_, NQV_>(gf_live);
    }
    template <bool LSRK>
    static Kernel tendency_recv(bool gf, bool recv)
    {
        return recv ? tendency_kernel<P, NQ_, NQV_, LSRK, true>(gf) : tendency_kernel<P, NQ_, NQV_, LSRK, false>(gf);
    }
    static Kernel pick_tendency(bool lsrk, bool gf, bool recv, GargOut out)
    {
        if (out != GargOut::none) {
            if constexpr (HO) {  // (handoff_eligible: fused update, no gradient flux, no ghosts)
                if constexpr (ELIDE)
                    if (out == GargOut::records) return k_tendency<P, NQ_, NQV_, true, false, false, true, false>;
                return k_tendency<P, NQ_, NQV_, true, false, false, true>;
            }
            return nullptr;
        }
        return lsrk ? tendency_recv<true>(gf, recv) : tendency_recv<false>(gf, recv);
    }
    // The Laplacian and gradient-of-Laplacian passes of an evaluation that reads the records (c.garg_in)
    // hand the Laplacians on as ring-ordered records (cmdg_common.h ring_slot); the second gathers
    // them through facePr.
    // fused (RhsCtx::lap_fused): the launch does the work of the gradient pass as well, which is then
    // not launched (k_lapfused).
    // A law without hyperdiffusive states has neither pass (rhs_segment's `hyper`), and only a hand-off
    // law has the ring-ordered ones.
    static Kernel pick_divgrad(bool ring, bool fused)
    {
        if constexpr (HO) {
            if (ring && fused) return k_lapfused<P, NQ_, NQV_>;
            if (ring) return k_divgrad<P, NQ_, NQV_, true>;
        }
        if constexpr (P::NHYP > 0)
            if (!ring && !fused) return k_divgrad<P, NQ_, NQV_>;
        return nullptr;
    }
    static Kernel pick_gradlap(bool ring)
    {
        if constexpr (HO)
            if (ring) return k_gradlap<P, NQ_, NQV_, true>;
        if constexpr (P::NHYP > 0)
            if (!ring) return k_gradlap<P, NQ_, NQV_>;
        return nullptr;
    }
    int launch_gradients(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) override
    {
        if (c.lap_fused) return CMDG_OK;  // (formed inside the Laplacian launch)
        return in_pass(GRADIENTS, n, exterior, st, [&] {
            const PassArgs<P> args = make_args(c, elems, n, diffusion_direction, exterior,
                                               gf_live() ? slot[SLOT_GF].sendbuf : nullptr,
                                               ngl > 0 ? slot[SLOT_HG].sendbuf : nullptr);
            return launch_picked(pick_gradients(gf_live(), c.garg_in), (unsigned)n, KDims<NQ_, NQV_>::NT, st, args,
                                 "gradient", "gf_live = %d, garg_in = %d", (int)gf_live(), (int)c.garg_in);
        });
    }
    int launch_divgrad(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) override
    {
        return in_pass(DIVGRAD, n, exterior, st, [&] {
            PassArgs<P> args = make_args(c, elems, n, diffusion_direction, exterior, slot[SLOT_HD].sendbuf, nullptr);
            const bool fused = HO && c.garg_in && c.lap_fused;
            if (fused) {  // (the tables of k_lapfused travel in two arguments the pass does not read)
                args.g.facePr = d_lapI;
                args.derived = d_lapT;
            }
            return launch_picked(pick_divgrad(c.garg_in, fused), (unsigned)n, KDims<NQ_, NQV_>::NT, st, args,
                                 "Laplacian", "ring = %d, fused = %d", (int)c.garg_in, (int)fused);
        });
    }
    int launch_gradlap(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) override
    {
        return in_pass(GRADLAP, n, exterior, st, [&] {
            PassArgs<P> args = make_args(c, elems, n, diffusion_direction, exterior, slot[SLOT_HG].sendbuf, nullptr);
            if (c.garg_in) args.g.faceP = g.facePr;
            return launch_picked(pick_gradlap(c.garg_in), (unsigned)n, KDims<NQ_, NQV_>::NT, st, args,
                                 "gradient-of-Laplacian", "ring = %d", (int)c.garg_in);
        });
    }
    int launch_tendency(const RhsCtx &c, const int64_t *elems, int64_t n, bool exterior, hipStream_t st) override
    {
        return in_pass(TENDENCY, n, exterior, st, [&] {
            using SH = TendencyShape<P, NQ_, NQV_>;
            PassArgs<P> args = make_args(c, elems, n, direction, exterior, c.lsrk ? slot[SLOT_Q].sendbuf : nullptr, nullptr);
            const bool recv = args.h.ghostslot != nullptr && exterior;  // (interior elements have no ghost neighbour)
            if (!recv) args.h.ghostslot = nullptr;
            const bool gf = needs_gradflux<P>(prm);
            return launch_picked(pick_tendency(c.lsrk, gf, recv, c.garg_out), (unsigned)SH::blocks(n), SH::NT, st, args,
                                 "tendency", "lsrk = %d, gradient flux = %d, recv = %d, garg_out = %d", (int)c.lsrk,
                                 (int)gf, (int)recv, (int)c.garg_out);
        });
    }
};

template <class P, int NQ_, int NQV_ = NQ_>
EngineBase *make_engine(const cmdg_desc *d)
{
    auto *e = new EngineT<P, NQ_, NQV_>();
    e->init_law(d);
    return e;
}

// The laws compiled in are the rows of one table (create.hip LAWS), their factories are declared in
// laws.h and defined per physics family in the engine_*.hip units.

}  // namespace cmdg
