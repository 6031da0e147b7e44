// kernel_params.hip — kernel-parameter construction: covgram_kernel (include/covgram.h) -> HostKernel (common.hpp), the double-precision
// master copy of the parameter block every device kernel receives.
#include <algorithm>

#include "driver.hpp"

namespace covgram {

// ------------------------------------------------------------------------------------------------
// kernel parameters.  MaternP tables follow src/stationary.jl:117-191 (coefficients :184-191,
// normalisation :157, derivatives at zero :172-182 — derived from the power series, not SymEngine).
// ------------------------------------------------------------------------------------------------
static long double factl(int n) {
    long double f = 1;
    for (int i = 2; i <= n; ++i) f *= i;
    return f;
}

// normalised polynomial h[m], m = 0..q:  H_q(r) = exp(-r) sum_m h[m] r^m,  H_q(0) = 1
static void maternp_poly(int q, long double* h) {
    const long double nrm = factl(2 * q) / factl(q);
    for (int m = 0; m <= q; ++m) {
        // coefficient of (2r)^m: (2q-m)! / (m! (q-m)!)
        const long double c = factl(2 * q - m) / (factl(m) * factl(q - m));
        h[m] = c * powl(2.0L, m) / nrm;
    }
}

// d_i = d^i/ds^i MaternP_p(s) at s = 0 (i = 1..p): the r^(2i) series coefficient of exp(-r) q_p(r) times (2p+1)^i i!
static void maternp_derivs0(int p, long double* d /* d[1..p] */) {
    long double h[MAXP + 1];
    maternp_poly(p, h);
    for (int i = 1; i <= p; ++i) {
        long double coef = 0;
        for (int m = 0; m <= std::min(p, 2 * i); ++m) {
            const int k = 2 * i - m;
            coef += h[m] * (((k & 1) ? -1.0L : 1.0L) / factl(k));
        }
        d[i] = coef * powl((long double)(2 * p + 1), i) * factl(i);
    }
}

static int make_simple_kernel(const covgram_kernel* k, int dtype, bool for_gradient, HostKernel* out);

// Composite: every factor keeps its own parameter block with gamma = 1/l (unfolded EQ); rows and columns stay unscaled.
// mixed (the composites of covgram_grad_mvm_mixed, grad_mixed.hpp, and of covgram_mvm_mixed / covgram_matrix_mixed, mixed_mvm.hpp): the head's
// trait binds nobody, every factor is validated on its OWN trait and a NeuralNetwork factor keeps sigma in fkp.param; the gradient mode
// refuses the leaves without a jet in (x.y, |x|^2, |y|^2), the values mode takes every leaf, the parameters mode (covgram_bilinear_grad_mixed,
// mixed_bilin_grad.hip) every leaf but Matern(nu).
int make_composite_kernel(const covgram_kernel_composite* c, int dtype, CompositeMode mode, HostKernel* out) {
    const covgram_kernel& h = c->head;
    const bool mixed = mode != COMPOSITE_ONE_TRAIT;
    if (mixed)
        CG_REQUIRE(h.family == COVGRAM_COMPOSITE, COVGRAM_EINVAL, "%s takes a covgram_kernel_composite (head.family = %d)",
                   mode == COMPOSITE_MIXED_GRADIENT ? "covgram_grad_mvm_mixed"
                   : mode == COMPOSITE_MIXED_PARAMETERS ? "covgram_bilinear_grad_mixed" : "covgram_mvm_mixed / covgram_matrix_mixed", h.family);
    else CG_REQUIRE(h.trait == COVGRAM_ISOTROPIC || h.trait == COVGRAM_DOTPRODUCT, COVGRAM_EINVAL, "composite: bad trait %d", h.trait);
    CG_REQUIRE(h.power == 1 && h.lengthscale == 1.0, COVGRAM_EINVAL, "composite head must have power == 1 and lengthscale == 1");
    CG_REQUIRE(c->nterms >= 1 && c->nterms <= EXPR_MAXT, COVGRAM_EUNSUPPORTED, "composite: %d terms (1..%d supported)", c->nterms, EXPR_MAXT);
    memset(out, 0, sizeof(*out));
    out->k = h;
    out->kp.gamma = 1.0; out->kp.gamma2 = 1.0; out->kp.scale = h.scale; out->kp.power = 1;
    out->eq_folded = false;
    out->tu_family = (!mixed && h.trait == COVGRAM_ISOTROPIC) ? FAM_EXPR_ISO : FAM_EXPR_DOT;
    out->nterms = c->nterms;
    int nin = 0, nf = 0;   // factors consumed from the descriptor / profile factors kept for the device
    for (int t = 0; t < c->nterms; ++t) {
        CG_REQUIRE(c->nfactors[t] >= 1, COVGRAM_EINVAL, "composite: term %d has no factors", t);
        out->nfac[t] = 0;
        out->coef[t] = 1.0;
        for (int f = 0; f < c->nfactors[t]; ++f, ++nin) {
            CG_REQUIRE(nin < EXPR_MAXF, COVGRAM_EUNSUPPORTED, "composite: more than %d factors", EXPR_MAXF);
            const covgram_kernel& fk = c->factors[nin];
            if (fk.family == COVGRAM_CONSTANT) {   // Constants fold into the term's coefficient
                out->coef[t] *= fk.scale;
                continue;
            }
            KParams<double>& kp = out->fkp[nf];
            if (mixed && fk.family == COVGRAM_NEURALNETWORK) {
                CG_REQUIRE(fk.param >= 0, COVGRAM_EINVAL, "DomainError: NeuralNetwork sigma = %g is negative", fk.param);
                CG_REQUIRE(fk.power >= 1, COVGRAM_EINVAL, "Power exponent must be >= 1 (got %d)", fk.power);
                CG_REQUIRE(fk.lengthscale == 1.0, COVGRAM_EINVAL, "Lengthscale applies to isotropic kernels only");
                kp.gamma = 1.0; kp.gamma2 = 1.0; kp.param = fk.param; kp.power = fk.power;
            } else {
                if (mixed) CG_REQUIRE(fk.family >= 0 && fk.family < COVGRAM_NFAMILY, COVGRAM_EUNSUPPORTED, "unknown kernel family %d", fk.family);
                if (mode == COMPOSITE_MIXED_GRADIENT) {
                    const char* name = kFamilyNames[fk.family];
                    CG_REQUIRE(fk.family != COVGRAM_EXP && fk.family != COVGRAM_GAMMAEXP && !(fk.family == COVGRAM_MATERNP && fk.p == 0), COVGRAM_EUNSUPPORTED,
                               "mixed gradient kernel: the leaf %s%s is singular at zero distance and has no device path here", name,
                               fk.family == COVGRAM_MATERNP ? "(0)" : "");
                    CG_REQUIRE(fk.family != COVGRAM_MATERN, COVGRAM_EUNSUPPORTED, "mixed gradient kernel: the leaf %s(nu) has no device path here (MaternP does)", name);
                } else if (mode == COMPOSITE_MIXED_PARAMETERS) {
                    CG_REQUIRE(fk.family != COVGRAM_MATERN, COVGRAM_EUNSUPPORTED,
                               "bilinear_grad_mixed: the leaf %s with real nu is not supported (half-integer nu: MaternP)", kFamilyNames[fk.family]);
                } else if (!mixed) {
                    CG_REQUIRE(fk.trait == h.trait, COVGRAM_EINVAL, "composite: factor %d has trait %d, head has %d (GenericInput is not a device path)",
                               nin, fk.trait, h.trait);
                }
                HostKernel one;
                int rc = make_simple_kernel(&fk, dtype, true, &one);   // the factor's own trait against its family, its parameters
                if (rc) return rc;
                kp = one.kp;
            }
            kp.scale = 1.0;
            out->coef[t] *= fk.scale;              // (scale * phi)^1 only: a factor's scale multiplies the term once
            out->ffam[nf] = fk.family;
            ++out->nfac[t]; ++nf;
        }
    }
    return COVGRAM_OK;
}

int make_host_kernel(const covgram_kernel* k, int dtype, bool for_gradient, HostKernel* out) {
    CG_REQUIRE(k != nullptr, COVGRAM_EINVAL, "kernel is NULL");
    if (k->family == COVGRAM_COMPOSITE) return make_composite_kernel((const covgram_kernel_composite*)k, dtype, COMPOSITE_ONE_TRAIT, out);
    return make_simple_kernel(k, dtype, for_gradient, out);
}

static int make_simple_kernel(const covgram_kernel* k, int dtype, bool for_gradient, HostKernel* out) {
    CG_REQUIRE(k->family >= 0 && k->family < COVGRAM_NFAMILY, COVGRAM_EUNSUPPORTED, "unknown kernel family %d", k->family);
    if (k->family == COVGRAM_MATERNP && k->p == 0 && !for_gradient) {
        // MaternP(0)(s) = exp(-sqrt(s)) IS the Exponential profile (src/stationary.jl:117-158 with p = 0; tests/golden closed forms): the
        // value-only kernels run it as such instead of through the general MaternP body (fp32 n = 32768: 436 -> 293 us, profiles/r04_sym32_sweep.txt)
        covgram_kernel e = *k;
        e.family = COVGRAM_EXP; e.p = 0; e.param = 0.0;
        return make_simple_kernel(&e, dtype, for_gradient, out);
    }
    const bool dotfam = (k->family == COVGRAM_DOT || k->family == COVGRAM_EXPDOT || k->family == COVGRAM_ASINDOT);
    const int trait = dotfam ? COVGRAM_DOTPRODUCT : COVGRAM_ISOTROPIC;
    CG_REQUIRE(k->trait == trait, COVGRAM_EINVAL, "kernel trait %d does not match family %d (input_trait would be %d)",
               k->trait, k->family, trait);
    CG_REQUIRE(k->power >= 1, COVGRAM_EINVAL, "Power exponent must be >= 1 (got %d)", k->power);
    CG_REQUIRE(k->lengthscale > 0, COVGRAM_EINVAL, "DomainError: l = %g is non-positive", k->lengthscale);
    CG_REQUIRE(!(dotfam && k->lengthscale != 1.0), COVGRAM_EINVAL, "Lengthscale applies to isotropic kernels only");
    memset(out, 0, sizeof(*out));
    out->k = *k;
    out->tu_family = k->family;
    KParams<double>& kp = out->kp;
    const double inv_l = 1.0 / k->lengthscale;
    kp.scale = k->scale;
    kp.power = k->power;
    kp.p = 0;
    kp.gamma = dotfam ? 1.0 : inv_l;
    kp.c0 = 0;
    out->eq_folded = false;
    const double LOG2E = 1.4426950408889634074;
    switch (k->family) {
        case COVGRAM_EQ:
            kp.c0 = -0.5 * LOG2E;  // exp(-s/2) = exp2(c0 s)
            if (!for_gradient) {     // dense path: fold sqrt(log2(e)/2) into the coordinate pre-scale
                kp.gamma = inv_l * sqrt(0.5 * LOG2E);
                out->eq_folded = true;
            }
            break;
        case COVGRAM_EXP:
            // fp32 dense path: fold log2(e) into the coordinate pre-scale, exp(-r) = exp2(-sqrt(s')) (profiles.hpp: dense_folded)
            if (!for_gradient && dtype == COVGRAM_F32) { kp.gamma = inv_l * LOG2E; out->eq_folded = true; }
            break;
        case COVGRAM_RQ:
            CG_REQUIRE(k->param > 0, COVGRAM_EINVAL, "DomainError: alpha not positive");
            kp.param = k->param;
            kp.c0 = 1.0 / (2.0 * k->param);
            break;
        case COVGRAM_GAMMAEXP:
            CG_REQUIRE(k->param >= 0 && k->param <= 2, COVGRAM_EINVAL, "DomainError: gamma not in [0,2]");
            kp.param = 0.5 * k->param;
            break;
        case COVGRAM_IMQ:
            kp.param = k->param * k->param;
            break;
        case COVGRAM_MATERNP: {
            CG_REQUIRE(k->p >= 0, COVGRAM_EINVAL, "DomainError: p = %d is negative", k->p);
            CG_REQUIRE(k->p <= MAXP, COVGRAM_EUNSUPPORTED, "MaternP order %d exceeds the compiled maximum %d", k->p, MAXP);
            const int p = k->p;
            kp.p = p;
            kp.mp_c = 2.0 * p + 1.0;
            long double h[MAXP + 1], d[MAXP + 1];
            maternp_poly(p, h);
            for (int m = 0; m <= p; ++m) kp.h0[m] = (double)h[m];
            if (p >= 1) { maternp_poly(p - 1, h); for (int m = 0; m <= p - 1; ++m) kp.h1[m] = (double)h[m]; }
            if (p >= 2) { maternp_poly(p - 2, h); for (int m = 0; m <= p - 2; ++m) kp.h2[m] = (double)h[m]; }
            kp.ty[0] = 1.0;
            if (p >= 1) {
                maternp_derivs0(p, d);
                for (int i = 1; i <= p; ++i) kp.ty[i] = (double)(d[i] / factl(i));
                kp.mp_d1 = (double)d[1];
                kp.mp_d2 = (p >= 2) ? (double)d[2] : 0.0;
                const double eps = (dtype == COVGRAM_F64) ? 2.220446049250313e-16 : 1.1920928955078125e-07;
                kp.mp_bound = pow(eps, 1.0 / p);     // src/stationary.jl:135
            } else {
                kp.mp_bound = 0.0;                   // eps^(1/0) = 0: never taken
            }
            if (!for_gradient) {
                // dense path: fold sqrt(2p+1) and log2(e) into the coordinate pre-scale, s' = (2p+1) log2(e)^2 s / l^2, so that
                // sqrt(s') = r log2(e): H_p(r) = exp2(-sqrt(s')) sum_m (h_m / log2(e)^m) sqrt(s')^m, Taylor in s'
                const double f2 = kp.mp_c * LOG2E * LOG2E;
                kp.gamma = inv_l * sqrt(f2);
                double li = 1.0, fi = 1.0;
                for (int i = 0; i <= p; ++i) { kp.h0[i] *= li; kp.ty[i] *= fi; li /= LOG2E; fi /= f2; }
                kp.mp_bound *= f2;
                out->eq_folded = true;
            }
            break;
        }
        case COVGRAM_MATERN: {
            // Matern(nu), real nu > 0 (src/stationary.jl:87-114): phi = C r^nu K_nu(r), r = sqrt(2 nu s), C = 2^(1-nu)/Gamma(nu);
            // below taylor_bound the reference's polynomial (:100-110).  K_a by Temme's series (x < 2) / Steed's continued fraction
            // (x >= 2) at order mu = a - round(a) and upward recurrence; the mu-only constants are computed here, per order:
            // h0 <- order nu (value), h1 <- |nu - 1| (phi'), h2 <- |nu - 2| (phi'').
            const double nu = k->param;
            CG_REQUIRE(nu > 0, COVGRAM_EINVAL, "DomainError: nu = %g is negative", nu);
            CG_REQUIRE(nu <= 64, COVGRAM_EUNSUPPORTED, "Matern: nu = %g exceeds 64", nu);
            kp.param = nu;
            kp.mp_c = 2.0 * nu;
            const double eps = (dtype == COVGRAM_F64) ? 2.220446049250313e-16 : 1.1920928955078125e-07;
            kp.mp_bound = (nu > 2) ? sqrt(eps) : ((nu > 1) ? eps : 0.0);
            kp.ty[0] = 1.0;
            kp.ty[1] = (nu > 1) ? nu / (2 * (1 - nu)) : 0.0;
            kp.ty[2] = (nu > 2) ? nu * nu / (8 * (2 - 3 * nu + nu * nu)) : 0.0;
            kp.c0 = exp2(1.0 - nu) / tgamma(nu);                      // C
            auto order = [&](double a, double* h) {                   // h[0..6] = nl, mu, gam1, gam2, 1/Gamma(1+mu), 1/Gamma(1-mu), pi mu / sin(pi mu)
                const double nl = floor(a + 0.5);
                const long double mu = (long double)a - nl;
                const long double gp = 1.0L / tgammal(1.0L + mu), gm = 1.0L / tgammal(1.0L - mu);
                long double g1;
                if (fabsl(mu) < 0.01L) {                              // (1/Gamma(1-mu) - 1/Gamma(1+mu)) / (2 mu) from the series of 1/Gamma
                    const long double m2 = mu * mu;
                    g1 = -(0.57721566490153286061L + m2 * (-0.042002635034095235529L + m2 * (-0.042197734555544336748L + m2 * 0.0072189432466630995424L)));
                } else {
                    g1 = (gm - gp) / (2 * mu);
                }
                const long double pimu = 3.14159265358979323846264338327950288L * mu;
                h[0] = nl; h[1] = (double)mu; h[2] = (double)g1; h[3] = (double)((gm + gp) / 2); h[4] = (double)gp; h[5] = (double)gm;
                h[6] = (fabsl(pimu) < 1e-18L) ? 1.0 : (double)(pimu / sinl(pimu));
            };
            order(nu, kp.h0); order(fabs(nu - 1), kp.h1); order(fabs(nu - 2), kp.h2);
            break;
        }
        default: break;
    }
    kp.gamma2 = kp.gamma * kp.gamma;
    return COVGRAM_OK;
}

}  // namespace covgram

using namespace covgram;

extern "C" {

// debugging / test hook: the double-precision parameter block the device kernels receive.
// out[0..8] = gamma, gamma2, scale, param, c0, mp_c, mp_bound, mp_d1, mp_d2; then h0, h1, h2, ty (9 each).
int covgram_debug_kernel_params(const covgram_kernel* k, int32_t dtype, int32_t for_gradient, double* out45) {
    HostKernel hk;
    int rc = make_host_kernel(k, dtype, for_gradient != 0, &hk);
    if (rc) return rc;
    CG_REQUIRE(out45 != nullptr, COVGRAM_EINVAL, "out is NULL");
    const KParams<double>& p = hk.kp;
    double* o = out45;
    *o++ = p.gamma; *o++ = p.gamma2; *o++ = p.scale; *o++ = p.param; *o++ = p.c0; *o++ = p.mp_c; *o++ = p.mp_bound; *o++ = p.mp_d1; *o++ = p.mp_d2;
    for (int i = 0; i <= MAXP; ++i) *o++ = p.h0[i];
    for (int i = 0; i <= MAXP; ++i) *o++ = p.h1[i];
    for (int i = 0; i <= MAXP; ++i) *o++ = p.h2[i];
    for (int i = 0; i <= MAXP; ++i) *o++ = p.ty[i];
    return COVGRAM_OK;
}

}  // extern "C"
