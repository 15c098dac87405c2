// One row of H_h psi from the handle's operator tables: what adjoint_apply_operator_kernel (adjoint.hip) and
// operator_moments_kernel (moments.hip) both form.  The row comes back by value: with reference parameters in their place the
// compiler pairs the two products of the adjoint kernel's Re<psi|lambda> the other way round in their fused multiply-add, and
// that call's values would no longer be the bits they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace qsv {

// lambda_i = D[i] psi_i + sum over x-mask groups of (w_re(i) - i w_im(i)) psi_(i ^ x), with w_re / w_im(i) the sums of
// (-1)^popcount(i & z_k) coef_k over the group's terms with an even / odd number of Y factors (coef_k carries
// (-1)^floor(ny / 2), as pauli_groups_kernel reads it): P_k psi = (-i)^ny (-1)^popcount(i & z) psi_(i ^ x).  `st` is the state,
// `a` its amplitude i (the caller has loaded it), `diag` may be null.  The term tables are read at wave-uniform addresses.
struct OperatorRow {
    double re, im;
};
template <typename amp>
__device__ __forceinline__ OperatorRow operator_row(const amp* __restrict__ st, unsigned long long i, amp a, const double* __restrict__ diag,
                                             int n_groups, const PauliGroup* __restrict__ groups, const uint64_t* __restrict__ term_z,
                                             const double* __restrict__ term_coef, const uint32_t* __restrict__ term_odd) {
    double l_re = 0.0, l_im = 0.0;
    if (diag) {
        const double d = diag[i];
        l_re = d * double(a.re);
        l_im = d * double(a.im);
    }
    for (int g = 0; g < n_groups; ++g) {
        const PauliGroup gr = groups[g];
        const amp b = st[i ^ gr.x];
        double w_re = 0.0, w_im = 0.0;
        for (uint32_t k = gr.first; k < gr.first + gr.count; ++k) {
            const bool minus = __popcll(i & term_z[k]) & 1;
            const double c = minus ? -term_coef[k] : term_coef[k];
            if (term_odd[k])
                w_im += c;
            else
                w_re += c;
        }
        l_re += w_re * double(b.re) + w_im * double(b.im);
        l_im += w_re * double(b.im) - w_im * double(b.re);
    }
    return OperatorRow{l_re, l_im};
}

}  // namespace qsv
