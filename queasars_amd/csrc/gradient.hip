// Parameter-shift gradients: shift plan (host), the expansion / combination kernels and the Adam step (gradient.hpp).
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

// One wave per run.  Each lane takes the variables j = lane, lane + 64, ...: moments, update, the run's entry of x.  With a
// tolerance the squares of a round's updates go from lane to lane in ascending j (every lane holds the same running sum), so
// the norm is the sum a sequential loop forms.  Division and square root of doubles are correctly rounded (no fast-math), and
// nothing is contracted: the bits are NumPy's.
__global__ void __launch_bounds__(64) adam_step_kernel(const qsv_adam_step_args a) {
#pragma clang fp contract(off)
    const int r = blockIdx.x, lane = threadIdx.x;
    if (a.active[r] == 0) return;  // (the whole wave: a stopped run keeps every bit)
    const int size = a.sizes[r];
    if (size < 1 || size > a.columns_stride || size > a.grad_width) return;  // (the caller's error, qsv.h: the run is left alone)
    double* x = a.x + size_t(r) * size_t(a.width);
    double* m = a.m + size_t(r) * size_t(a.grad_width);
    double* v = a.v + size_t(r) * size_t(a.grad_width);
    const double* gradient = a.gradient + size_t(r) * size_t(a.grad_width);
    const int* columns = a.columns + size_t(r) * size_t(a.columns_stride);
    double sum = 0.0;
    for (int first = 0; first < size; first += 64) {  // (size is the wave's: every lane makes every round)
        const int j = first + lane;
        double square = 0.0;
        if (j < size) {
            const double g = gradient[j];
            const double m_new = a.beta_1 * m[j] + a.one_minus_beta_1 * g;
            const double v_new = a.beta_2 * v[j] + a.one_minus_beta_2 * (g * g);
            const double m_hat = m_new / a.bias_1;
            const double v_hat = v_new / a.bias_2;
            const double u = a.lr * m_hat / (sqrt(v_hat) + a.eps);
            m[j] = m_new;
            v[j] = v_new;
            const int col = columns[j];
            if (col >= 0 && col < a.width) x[col] = x[col] - u;
            square = u * u;
        }
        if (a.tol > 0.0) {
            const int count = size - first < 64 ? size - first : 64;
            for (int k = 0; k < count; ++k) sum = sum + __shfl(square, k, 64);
        }
    }
    if (lane == 0) {
        const long long done = a.iterations[r] + 1;
        a.iterations[r] = done;
        bool stop = done >= a.maxiter;
        if (a.tol > 0.0 && sqrt(sum) < a.tol) stop = true;
        if (stop) a.active[r] = 0;
    }
}

}  // namespace

hipError_t launch_adam_step(const qsv_adam_step_args& args, hipStream_t stream) {
    if (args.n_runs <= 0 || args.width <= 0) return hipSuccess;
    hipLaunchKernelGGL(adam_step_kernel, dim3(unsigned(args.n_runs)), dim3(64), 0, stream, args);
    return hipGetLastError();
}

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
