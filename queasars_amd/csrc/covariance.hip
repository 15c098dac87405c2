// Second moments of an observable set (covariance.hpp).  A workgroup is one wave.  It takes 64 consecutive
// amplitudes at a time and one pair (a, b) of 16-observable blocks, forms lambda_m(i) = (O_m psi)_i for the 16 observables of
// block a into an LDS panel [observable][amplitude], and accumulates the 16 x 16 tile Re(Lambda_a^H Lambda_b) on the fp64 matrix
// pipe: v_mfma_f64_16x16x4_f64 sums over four amplitudes per instruction, real and imaginary parts as separate steps.  For
// a < b the wave keeps block a's operands in registers and forms block b's panel in the same LDS.  E_m = Re<psi|lambda_m> is summed
// beside it in one register per lane, from the same operands and psi in a 17th panel row (diagonal pairs).  Every sum is fp64 whatever the
// state's type and runs in a fixed order: per workgroup over its amplitudes in ascending order, across workgroups in ascending
// order in the combine kernel.  No floating-point atomics.
#include "covariance.hpp"

namespace qsv {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

template <typename real>
struct alignas(2 * sizeof(real)) ccx {  // (one load per amplitude)
    real re, im;
};

constexpr uint32_t kRow = 66;  // doubles per panel row: lanes m = 0 .. 15 read 8-byte words 4 m + 2 k apart, every bank once

// block pair p -> (a, b), a <= b
__device__ __forceinline__ void pair_blocks(uint32_t p, uint32_t n_blk, uint32_t& a, uint32_t& b) {
    a = 0;
    while (p >= n_blk - a) {
        p -= n_blk - a;
        ++a;
    }
    b = a + p;
}
// the pair (a, a)
__device__ __forceinline__ uint32_t diagonal_pair(uint32_t a, uint32_t n_blk) { return a * n_blk - a * (a - 1) / 2; }

// lambda_m(i) for the observables m = 16 blk + j of one block into the panel rows j, for the lane's amplitude i (`live`: i is
// inside the state; the other lanes write zeros).  The control flow and the table addresses are the same in every lane.
template <typename real>
__device__ __forceinline__ void fill_panel(const ccx<real>* __restrict__ st, unsigned long long i, bool live, uint32_t blk, uint32_t n_obs,
                                           const uint32_t* __restrict__ obs_first, const PauliGroup* __restrict__ groups,
                                           const CovTerm* __restrict__ terms, double* __restrict__ p_re, double* __restrict__ p_im,
                                           uint32_t lane) {
    for (uint32_t j = 0; j < kCovBlock; ++j) {
        const uint32_t m = blk * kCovBlock + j;
        double l_re = 0.0, l_im = 0.0;
        if (m < n_obs) {
            const uint32_t g1 = obs_first[m + 1];
            for (uint32_t g = obs_first[m]; g < g1; ++g) {
                const PauliGroup gr = groups[g];
                ccx<real> b{real(0), real(0)};
                if (live) b = st[i ^ gr.x];
                double w_re = 0.0, w_im = 0.0;
                for (uint32_t k = gr.first; k < gr.first + gr.count; ++k) {
                    const CovTerm t = terms[k];
                    const uint32_t flip = uint32_t(__popcll(i & t.z)) << 31;  // (-1)^popcount(i & z) as the sign bit (bit 63 of z meets no bit of i)
                    const double c = __hiloint2double(__double2hiint(t.c) ^ int(flip), __double2loint(t.c));
                    if (t.z & kCovOddY)
                        w_im += c;
                    else
                        w_re += c;
                }
                l_re += w_re * double(b.re) + w_im * double(b.im);
                l_im += w_re * double(b.im) - w_im * double(b.re);
            }
        }
        p_re[j * kRow + lane] = l_re;
        p_im[j * kRow + lane] = l_im;
    }
}

template <typename real>
__global__ void __launch_bounds__(64)
covariance_panels_kernel(const ccx<real>* __restrict__ states, unsigned long long dim, uint32_t n_obs, const uint32_t* __restrict__ obs_first,
                         const PauliGroup* __restrict__ groups, const CovTerm* __restrict__ terms, double* __restrict__ partials) {
    __shared__ double p_re[(kCovBlock + 1) * kRow], p_im[(kCovBlock + 1) * kRow];  // (row 16: psi itself)
    const uint32_t lane = threadIdx.x, pos = blockIdx.z, n_blk = (n_obs + kCovBlock - 1) / kCovBlock;
    uint32_t blk_a, blk_b;
    pair_blocks(blockIdx.y, n_blk, blk_a, blk_b);
    const bool diagonal = blk_a == blk_b;
    const ccx<real>* st = states + size_t(pos) * dim;
    // lane l supplies the operand element (amplitude 4 s + (l >> 4) of the 64, observable l & 15) at step s
    const uint32_t at = (lane & 15) * kRow + (lane >> 4);
    v4d acc_re = {0.0, 0.0, 0.0, 0.0}, acc_im = {0.0, 0.0, 0.0, 0.0};
    double e = 0.0;  // the lane's share of Re<psi|lambda_m>, m = lane & 15: the amplitudes 4 s + (lane >> 4) of every 64
    const unsigned long long chunks = (dim + 63) / 64;
    for (unsigned long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const unsigned long long i = chunk * 64 + lane;
        const bool live = i < dim;
        ccx<real> a{real(0), real(0)};
        if (live) a = st[i];
        fill_panel(st, i, live, blk_a, n_obs, obs_first, groups, terms, p_re, p_im, lane);
        p_re[kCovBlock * kRow + lane] = double(a.re);
        p_im[kCovBlock * kRow + lane] = double(a.im);
        __syncthreads();
        double a_re[16], a_im[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            a_re[s] = p_re[at + 4 * s];
            a_im[s] = p_im[at + 4 * s];
        }
        if (diagonal) {
#pragma unroll
            for (int s = 0; s < 16; ++s)
                e += a_re[s] * p_re[kCovBlock * kRow + (lane >> 4) + 4 * s] + a_im[s] * p_im[kCovBlock * kRow + (lane >> 4) + 4 * s];
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                acc_re = __builtin_amdgcn_mfma_f64_16x16x4f64(a_re[s], a_re[s], acc_re, 0, 0, 0);
                acc_im = __builtin_amdgcn_mfma_f64_16x16x4f64(a_im[s], a_im[s], acc_im, 0, 0, 0);
            }
        } else {
            __syncthreads();
            fill_panel(st, i, live, blk_b, n_obs, obs_first, groups, terms, p_re, p_im, lane);
            __syncthreads();
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                acc_re = __builtin_amdgcn_mfma_f64_16x16x4f64(a_re[s], p_re[at + 4 * s], acc_re, 0, 0, 0);
                acc_im = __builtin_amdgcn_mfma_f64_16x16x4f64(a_im[s], p_im[at + 4 * s], acc_im, 0, 0, 0);
            }
        }
        __syncthreads();  // (the next chunk's panel goes into the same LDS)
    }
    double* out = partials + ((size_t(pos) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kCovPartial;
    // C/D of the fp64 tile: column = lane & 15, row = (lane >> 4) + 4 * register
    const v4d acc = acc_re + acc_im;
    out[((lane >> 4) + 0) * 16 + (lane & 15)] = acc.x;
    out[((lane >> 4) + 4) * 16 + (lane & 15)] = acc.y;
    out[((lane >> 4) + 8) * 16 + (lane & 15)] = acc.z;
    out[((lane >> 4) + 12) * 16 + (lane & 15)] = acc.w;
    if (diagonal) {  // E_m: the four lanes m, m + 16, m + 32, m + 48, added in that pairing
        e += __shfl_xor(e, 16);
        e += __shfl_xor(e, 32);
        if (lane < kCovBlock) out[kCovBlock * kCovBlock + lane] = e;
    }
}

// One workgroup per (block pair, evaluation), one thread per entry of the tile.
__global__ void __launch_bounds__(256)
covariance_combine_kernel(const double* __restrict__ partials, uint32_t blocks, uint32_t n_obs, double* __restrict__ values,
                          double* __restrict__ cov) {
    __shared__ double e[2 * kCovBlock];
    const uint32_t t = threadIdx.x, pos = blockIdx.y, n_pairs = gridDim.x, n_blk = (n_obs + kCovBlock - 1) / kCovBlock;
    uint32_t blk_a, blk_b;
    pair_blocks(blockIdx.x, n_blk, blk_a, blk_b);
    const double* p = partials + (size_t(pos) * n_pairs + blockIdx.x) * blocks * kCovPartial;
    double g = 0.0;
    for (uint32_t w = 0; w < blocks; ++w) g += p[size_t(w) * kCovPartial + t];
    if (t < 2 * kCovBlock) {
        const uint32_t d = diagonal_pair(t < kCovBlock ? blk_a : blk_b, n_blk);
        const double* q = partials + (size_t(pos) * n_pairs + d) * blocks * kCovPartial + kCovBlock * kCovBlock + (t & 15);
        double s = 0.0;
        for (uint32_t w = 0; w < blocks; ++w) s += q[size_t(w) * kCovPartial];
        e[t] = s;
    }
    __syncthreads();
    const uint32_t r = t >> 4, c = t & 15, ma = blk_a * kCovBlock + r, mb = blk_b * kCovBlock + c;
    if (ma < n_obs && mb < n_obs && (blk_a != blk_b || r <= c)) {
        const double v = g - e[r] * e[kCovBlock + c];
        double* out = cov + size_t(pos) * n_obs * n_obs;
        out[size_t(ma) * n_obs + mb] = v;
        out[size_t(mb) * n_obs + ma] = v;
    }
    if (blk_a == blk_b && t < kCovBlock && blk_a * kCovBlock + t < n_obs) values[size_t(pos) * n_obs + blk_a * kCovBlock + t] = e[t];
}

}  // namespace

hipError_t launch_covariance_panels(int dtype, const void* states, int n_qubits, int n_evals, uint32_t n_obs, const uint32_t* obs_first,
                                    const PauliGroup* groups, const CovTerm* terms, double* partials, hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    const dim3 grid(covariance_blocks(n_qubits, n_obs), covariance_pairs(n_obs), unsigned(n_evals));
    const unsigned long long dim = 1ull << n_qubits;
    if (dtype == QSV_F64)
        hipLaunchKernelGGL(covariance_panels_kernel<double>, grid, dim3(64), 0, stream, static_cast<const ccx<double>*>(states), dim, n_obs,
                           obs_first, groups, terms, partials);
    else
        hipLaunchKernelGGL(covariance_panels_kernel<float>, grid, dim3(64), 0, stream, static_cast<const ccx<float>*>(states), dim, n_obs,
                           obs_first, groups, terms, partials);
    return hipGetLastError();
}

hipError_t launch_covariance_combine(const double* partials, int n_qubits, int n_evals, uint32_t n_obs, double* values, double* cov,
                                     hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    hipLaunchKernelGGL(covariance_combine_kernel, dim3(covariance_pairs(n_obs), unsigned(n_evals)), dim3(256), 0, stream, partials,
                       covariance_blocks(n_qubits, n_obs), n_obs, values, cov);
    return hipGetLastError();
}

}  // namespace qsv
