// Parameter-shift gradients: shift plan (host) and the expansion / combination kernels (gradient.hpp).
#include "gradient.hpp"

#include <vector>

namespace qsv {

int gradient_plan(int n_ops, const qsv_op* ops, int n_params, int32_t* out) {
    // per parameter: angle slots that read it, and whether one of them is theta of a cu3
    std::vector<int32_t> reads(size_t(n_params > 0 ? n_params : 0), 0);
    std::vector<char> four(reads.size(), 0);
    for (int i = 0; i < n_ops; ++i) {
        const qsv_op& o = ops[i];
        if (o.kind == QSV_OP_ID) continue;
        const int32_t slots[3] = {o.p_theta, o.p_phi, o.p_lambda};
        for (int s = 0; s < 3; ++s) {
            const int32_t p = slots[s];
            if (p < 0 || p >= n_params) continue;
            reads[size_t(p)] += 1;
            if (s == 0 && o.kind == QSV_OP_CU3) four[size_t(p)] = 1;
        }
    }
    int refused = 0;
    for (int p = 0; p < n_params; ++p) {
        out[p] = reads[size_t(p)] == 0 ? 0 : reads[size_t(p)] > 1 ? -1 : four[size_t(p)] ? 4 : 2;
        refused += out[p] < 0;
    }
    return refused;
}

namespace {

constexpr int kExpandRowsPerBlock = 4;  // one wave each

__global__ void __launch_bounds__(64 * kExpandRowsPerBlock)
gradient_expand_kernel(const double* __restrict__ base, long long base_stride, int base_width, const GradRow* __restrict__ rows,
                       long long n_rows, double* __restrict__ out, int out_width) {
    const long long r = (long long)blockIdx.x * kExpandRowsPerBlock + threadIdx.y;
    const int c = 2 * int(blockIdx.y * 64 + threadIdx.x);
    if (r >= n_rows || c >= out_width) return;  // (out_width is even: c + 1 < out_width as well)
    const GradRow row = rows[r];
    const double* src = base + (long long)row.base_row * base_stride;
    double2 v;
    v.x = c < base_width ? src[c] : 0.0;
    v.y = c + 1 < base_width ? src[c + 1] : 0.0;
    if (row.param == c) v.x = v.x + row.shift;
    if (row.param == c + 1) v.y = v.y + row.shift;
    *reinterpret_cast<double2*>(out + r * (long long)out_width + c) = v;
}

__global__ void __launch_bounds__(256)
gradient_combine_kernel(const double* __restrict__ values, const GradEntry* __restrict__ entries,
                        const long long* __restrict__ offsets, long long n_evals, int out_width, double cp, double cm,
                        double* __restrict__ out) {
#pragma clang fp contract(off)  // (every product and difference is rounded on its own, as NumPy's are)
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_evals * out_width) return;
    const long long e = idx / out_width;
    const long long j = idx - e * out_width;
    const long long first = offsets[e];
    double g = 0.0;
    if (j < offsets[e + 1] - first) {
        const GradEntry en = entries[first + j];
        const double* v = values + en.first_value;
        if (en.n_terms == 2) {
            const double d = v[0] - v[1];
            g = 0.5 * d;
        } else if (en.n_terms == 4) {
            const double d1 = v[0] - v[1];
            const double d3 = v[2] - v[3];
            const double a = cp * d1;
            const double b = cm * d3;
            g = a - b;
        }
    }
    out[idx] = g;
}

}  // namespace

hipError_t launch_gradient_expand(const double* base, int64_t base_stride, int base_width, const GradRow* rows, int64_t n_rows,
                                  double* out, int out_width, hipStream_t stream) {
    if (n_rows <= 0 || out_width <= 0) return hipSuccess;
    if (out_width % 2 != 0 || reinterpret_cast<uintptr_t>(out) % 16 != 0) return hipErrorInvalidValue;
    const unsigned row_blocks = unsigned((n_rows + kExpandRowsPerBlock - 1) / kExpandRowsPerBlock);
    const unsigned col_blocks = unsigned((out_width / 2 + 63) / 64);
    hipLaunchKernelGGL(gradient_expand_kernel, dim3(row_blocks, col_blocks), dim3(64, kExpandRowsPerBlock), 0, stream, base,
                       (long long)base_stride, base_width, rows, (long long)n_rows, out, out_width);
    return hipGetLastError();
}

hipError_t launch_gradient_combine(const double* values, const GradEntry* entries, const int64_t* offsets, int64_t n_evals,
                                   int out_width, double cp, double cm, double* out, hipStream_t stream) {
    if (n_evals <= 0 || out_width <= 0) return hipSuccess;
    const long long total = (long long)n_evals * out_width;
    hipLaunchKernelGGL(gradient_combine_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, stream, values, entries,
                       reinterpret_cast<const long long*>(offsets), (long long)n_evals, out_width, cp, cm, out);
    return hipGetLastError();
}

}  // namespace qsv
