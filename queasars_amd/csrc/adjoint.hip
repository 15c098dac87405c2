// Adjoint gradients (adjoint.hpp): the kernels of the reverse sweep.  Every sum is fp64 and is formed in a
// fixed order -- per thread over its pairs, across a wave by a butterfly, across waves and workgroups in index order --, so an
// evaluation's numbers depend on nothing but its circuit, its point and the operator.  No floating-point atomics.
#include "adjoint.hpp"
#include "operator_row.hpp"

namespace qsv {

namespace {

template <typename real>
struct acx {
    real re, im;
};

template <typename real>
__device__ __forceinline__ acx<real> load_amp(const acx<real>* p, bool streaming) {
    typedef real vec2 __attribute__((ext_vector_type(2)));
    const vec2 v = streaming ? __builtin_nontemporal_load(reinterpret_cast<const vec2*>(p)) : *reinterpret_cast<const vec2*>(p);
    return acx<real>{v.x, v.y};
}
template <typename real>
__device__ __forceinline__ void store_amp(acx<real>* p, acx<real> a, bool streaming) {
    typedef real vec2 __attribute__((ext_vector_type(2)));
    vec2 v;
    v.x = a.re;
    v.y = a.im;
    if (streaming)
        __builtin_nontemporal_store(v, reinterpret_cast<vec2*>(p));
    else
        *reinterpret_cast<vec2*>(p) = v;
}

// every lane receives the sum of the wave's 64 values, added in the butterfly's order
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double block_sum(double v, double* red) {  // red: one double per wave of the 256 threads
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(kAdjointThreads)
adjoint_prepare_kernel(const AdjEval* __restrict__ evals, const AdjGate* __restrict__ gates, uint32_t max_gates,
                       const double* __restrict__ values, long long width, double* __restrict__ mats) {
    const uint32_t pos = blockIdx.y;
    const AdjEval ev = evals[pos];
    const uint32_t g = blockIdx.x * kAdjointThreads + threadIdx.x;
    if (g >= ev.n_gates) return;
    const AdjGate gt = gates[ev.gate_base + g];
    const double* row = values + (long long)ev.row * width;
    double a[3];
    for (int s = 0; s < 3; ++s) a[s] = gt.p[s] >= 0 ? row[gt.p[s]] : gt.lit[s];
    double s, c, ps, pc, ls, lc, ss, sc;
    sincos(0.5 * a[0], &s, &c);
    sincos(a[1], &ps, &pc);         // e^{i phi}
    sincos(a[2], &ls, &lc);         // e^{i lambda}
    sincos(a[1] + a[2], &ss, &sc);  // e^{i (phi + lambda)}
    double* m = mats + (size_t(pos) * max_gates + g) * kAdjointMatDoubles;
    // U = [[c, -e^{i lambda} s], [e^{i phi} s, e^{i (phi + lambda)} c]] (Qiskit's UGate); U^dagger, rows as (re, im) pairs
    m[0] = c,        m[1] = 0.0,      m[2] = pc * s,  m[3] = -ps * s;
    m[4] = -lc * s,  m[5] = ls * s,   m[6] = sc * c,  m[7] = -ss * c;
    // dU/dtheta = 1/2 [[-s, -e^{i lambda} c], [e^{i phi} c, -e^{i (phi + lambda)} s]]
    m[8] = -0.5 * s,        m[9] = 0.0,             m[10] = -0.5 * lc * c,  m[11] = -0.5 * ls * c;
    m[12] = 0.5 * pc * c,   m[13] = 0.5 * ps * c,   m[14] = -0.5 * sc * s,  m[15] = -0.5 * ss * s;
    // dU/dphi = [[0, 0], [i e^{i phi} s, i e^{i (phi + lambda)} c]]
    m[16] = 0.0,      m[17] = 0.0,     m[18] = 0.0,      m[19] = 0.0;
    m[20] = -ps * s,  m[21] = pc * s,  m[22] = -ss * c,  m[23] = sc * c;
    // dU/dlambda = [[0, -i e^{i lambda} s], [0, i e^{i (phi + lambda)} c]]
    m[24] = 0.0,  m[25] = 0.0,  m[26] = ls * s,   m[27] = -lc * s;
    m[28] = 0.0,  m[29] = 0.0,  m[30] = -ss * c,  m[31] = sc * c;
}

// lambda = H_h psi, row by row (operator_row.hpp), and each workgroup's share of Re<psi|lambda>.
template <typename real>
__global__ void __launch_bounds__(kAdjointThreads)
adjoint_apply_operator_kernel(const acx<real>* __restrict__ states, acx<real>* __restrict__ lambda, unsigned long long dim,
                              const double* __restrict__ diag, int n_groups, const PauliGroup* __restrict__ groups,
                              const uint64_t* __restrict__ term_z, const double* __restrict__ term_coef,
                              const uint32_t* __restrict__ term_odd, bool streaming, double* __restrict__ e_partials) {
    __shared__ double red[4];
    const uint32_t pos = blockIdx.y;
    const acx<real>* st = states + size_t(pos) * dim;
    acx<real>* lm = lambda + size_t(pos) * dim;
    double acc = 0.0;
    const unsigned long long stride = (unsigned long long)gridDim.x * kAdjointThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kAdjointThreads + threadIdx.x; i < dim; i += stride) {
        const acx<real> a = st[i];
        const OperatorRow row = operator_row(st, i, a, diag, n_groups, groups, term_z, term_coef, term_odd);
        const double l_re = row.re, l_im = row.im;
        acc += double(a.re) * l_re + double(a.im) * l_im;
        store_amp(lm + i, acx<real>{real(l_re), real(l_im)}, streaming);
    }
    const double total = block_sum(acc, red);
    if (threadIdx.x == 0) e_partials[size_t(pos) * gridDim.x + blockIdx.x] = total;
}

constexpr int kHighBits = kAdjointTileBits - kAdjointLowBits;
constexpr int kWaves = kAdjointThreads / 64;
constexpr int kRedPerWave = 3 * kAdjointMaxRunGates;

template <typename real>
constexpr size_t run_lds_bytes() {
    return 2 * (sizeof(acx<real>) << kAdjointTileBits) + size_t(kWaves) * kRedPerWave * sizeof(double);
}

// One run of the sweep.  A workgroup takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ...: psi and lambda of the tile into
// LDS, the run's gates last first -- psi_(g-1) = U^dagger psi_g, the derivative terms Re<lambda_g| dU/d(slot) |psi_(g-1)>,
// lambda_(g-1) = U^dagger lambda_g, pair by pair --, both tiles back.  A thread's pairs of a gate are p = tid, tid + 256, ...
// (p with a zero inserted at the target's tile bit is the pair's lower element), so consecutive lanes touch consecutive elements;
// for a target below the lanes of one LDS access group the upper half of the group takes the pair's elements in the other order,
// which spreads the group over all banks instead of the even (or odd) half of them.
template <typename real>
__global__ void __launch_bounds__(kAdjointThreads)
adjoint_run_kernel(acx<real>* __restrict__ states, acx<real>* __restrict__ lambda, int n_qubits, uint32_t run,
                   const AdjEval* __restrict__ evals, const AdjRunDesc* __restrict__ runs, const AdjGate* __restrict__ gates,
                   const double* __restrict__ mats, uint32_t max_gates, bool streaming, double* __restrict__ partials) {
    extern __shared__ __align__(16) unsigned char adjoint_lds[];
    __shared__ uint8_t tile_qubit[kAdjointTileBits], outer_qubit[64];
    const uint32_t pos = blockIdx.y;
    const AdjEval ev = evals[pos];
    if (run >= ev.n_runs) return;  // (the whole workgroup: this evaluation's sweep is over)
    const AdjRunDesc rd = runs[ev.run_base + run];
    const uint32_t n_gates = run + 1 == ev.n_runs ? ev.n_gates - rd.first_gate : rd.n_gates;
    const int tile_bits = n_qubits < kAdjointTileBits ? n_qubits : kAdjointTileBits;
    const uint32_t tile = 1u << tile_bits, n_pairs = tile >> 1;
    acx<real>* s_psi = reinterpret_cast<acx<real>*>(adjoint_lds);
    acx<real>* s_lam = s_psi + (size_t(1) << kAdjointTileBits);
    double* s_red = reinterpret_cast<double*>(s_lam + (size_t(1) << kAdjointTileBits));
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

    if (tid == 0) {
        int k = 0, j = 0;
        for (int q = 0; q < n_qubits; ++q) {
            if ((rd.mask >> q) & 1) {
                if (k < kAdjointTileBits) tile_qubit[k++] = uint8_t(q);
            } else {
                outer_qubit[j++] = uint8_t(q);
            }
        }
    }
    for (uint32_t i = tid; i < kWaves * kRedPerWave; i += kAdjointThreads) s_red[i] = 0.0;
    __syncthreads();
    // tile bit k >= kAdjointLowBits is this qubit (the low bits are themselves)
    uint32_t high_qubit[kHighBits];
#pragma unroll
    for (int k = 0; k < kHighBits; ++k) high_qubit[k] = kAdjointLowBits + k < tile_bits ? tile_qubit[kAdjointLowBits + k] : 0;
    const uint32_t low_mask = (1u << (tile_bits < kAdjointLowBits ? tile_bits : kAdjointLowBits)) - 1;
    auto spread = [&](uint32_t l) -> unsigned long long {
        unsigned long long g = l & low_mask;
#pragma unroll
        for (int k = 0; k < kHighBits; ++k) g |= (unsigned long long)((l >> (kAdjointLowBits + k)) & 1u) << high_qubit[k];
        return g;
    };
    const unsigned long long dim = 1ull << n_qubits;
    acx<real>* st = states + size_t(pos) * dim;
    acx<real>* lm = lambda + size_t(pos) * dim;
    const int outer_bits = n_qubits - tile_bits;
    const unsigned long long n_tiles = 1ull << outer_bits;
    // the lanes of one LDS access group: 16 for 16-byte elements, 32 for 8-byte ones
    constexpr uint32_t swap_bit = sizeof(acx<real>) == 16 ? 3 : 4;

    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        unsigned long long base = 0;
        for (int j = 0; j < outer_bits; ++j) base |= ((t >> j) & 1ull) << outer_qubit[j];
        for (uint32_t l = tid; l < tile; l += kAdjointThreads) {
            const unsigned long long off = base | spread(l);
            s_psi[l] = load_amp(st + off, streaming);
            s_lam[l] = load_amp(lm + off, streaming);
        }
        __syncthreads();
        for (uint32_t gl = 0; gl < n_gates; ++gl) {
            const uint32_t g = rd.first_gate + gl;
            const AdjGate gt = gates[ev.gate_base + g];
            const double* m = mats + (size_t(pos) * max_gates + g) * kAdjointMatDoubles;
            const real u00r = real(m[0]), u00i = real(m[1]), u01r = real(m[2]), u01i = real(m[3]);
            const real u10r = real(m[4]), u10i = real(m[5]), u11r = real(m[6]), u11i = real(m[7]);
            const uint32_t tpos = gt.tpos, tbit = 1u << tpos;
            const bool controlled = gt.cpos != QSV_NO_CONTROL;
            const uint32_t cbit = controlled ? 1u << gt.cpos : 0u;
            const bool swap = tpos <= swap_bit && ((lane >> swap_bit) & 1u);
            double acc[3] = {0.0, 0.0, 0.0};
            for (uint32_t p = tid; p < n_pairs; p += kAdjointThreads) {
                const uint32_t i0 = ((p >> tpos) << (tpos + 1)) | (p & (tbit - 1)), i1 = i0 | tbit;
                if (controlled && !(i0 & cbit)) continue;  // (control 0: identity, and the derivative's block is zero)
                const uint32_t ix = swap ? i1 : i0, iy = swap ? i0 : i1;
                const acx<real> px = s_psi[ix], py = s_psi[iy], lx = s_lam[ix], ly = s_lam[iy];
                const acx<real> a0 = swap ? py : px, a1 = swap ? px : py, l0 = swap ? ly : lx, l1 = swap ? lx : ly;
                // psi_(g-1) = U^dagger psi_g
                acx<real> b0, b1, k0, k1;
                b0.re = u00r * a0.re - u00i * a0.im + u01r * a1.re - u01i * a1.im;
                b0.im = u00r * a0.im + u00i * a0.re + u01r * a1.im + u01i * a1.re;
                b1.re = u10r * a0.re - u10i * a0.im + u11r * a1.re - u11i * a1.im;
                b1.im = u10r * a0.im + u10i * a0.re + u11r * a1.im + u11i * a1.re;
                // Re(conj(l0) w0 + conj(l1) w1), w = dU/d(slot) psi_(g-1)
                const double b0r = b0.re, b0i = b0.im, b1r = b1.re, b1i = b1.im;
                const double l0r = l0.re, l0i = l0.im, l1r = l1.re, l1i = l1.im;
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    if (gt.p[s] < 0) continue;
                    const double* d = m + 8 * (s + 1);
                    const double w0r = d[0] * b0r - d[1] * b0i + d[2] * b1r - d[3] * b1i;
                    const double w0i = d[0] * b0i + d[1] * b0r + d[2] * b1i + d[3] * b1r;
                    const double w1r = d[4] * b0r - d[5] * b0i + d[6] * b1r - d[7] * b1i;
                    const double w1i = d[4] * b0i + d[5] * b0r + d[6] * b1i + d[7] * b1r;
                    acc[s] += (l0r * w0r + l0i * w0i) + (l1r * w1r + l1i * w1i);
                }
                // lambda_(g-1) = U^dagger lambda_g
                k0.re = u00r * l0.re - u00i * l0.im + u01r * l1.re - u01i * l1.im;
                k0.im = u00r * l0.im + u00i * l0.re + u01r * l1.im + u01i * l1.re;
                k1.re = u10r * l0.re - u10i * l0.im + u11r * l1.re - u11i * l1.im;
                k1.im = u10r * l0.im + u10i * l0.re + u11r * l1.im + u11i * l1.re;
                s_psi[ix] = swap ? b1 : b0;
                s_psi[iy] = swap ? b0 : b1;
                s_lam[ix] = swap ? k1 : k0;
                s_lam[iy] = swap ? k0 : k1;
            }
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                if (gt.p[s] < 0) continue;  // (the gate's, so the whole workgroup's)
                const double sum = wave_sum(acc[s]);
                if (lane == 0) s_red[wave * kRedPerWave + 3 * gl + s] += sum;
            }
            __syncthreads();  // (the next gate pairs other elements)
        }
        for (uint32_t l = tid; l < tile; l += kAdjointThreads) {
            const unsigned long long off = base | spread(l);
            store_amp(st + off, s_psi[l], streaming);
            store_amp(lm + off, s_lam[l], streaming);
        }
        __syncthreads();  // (the next tile's loads overwrite what these stores read)
    }
    for (uint32_t i = tid; i < 3 * n_gates; i += kAdjointThreads) {
        double sum = 0.0;
        for (int w = 0; w < kWaves; ++w) sum += s_red[w * kRedPerWave + i];
        partials[(size_t(pos) * 3 * max_gates + 3 * rd.first_gate + i) * gridDim.x + blockIdx.x] = sum;
    }
}

// One wave per (evaluation, entry); entry out_width is the evaluation's value.
__global__ void __launch_bounds__(kAdjointThreads)
adjoint_combine_kernel(const AdjEval* __restrict__ evals, const long long* __restrict__ entry_offsets,
                       const AdjEntry* __restrict__ entries, const uint32_t* __restrict__ slots, const double* __restrict__ partials,
                       uint32_t max_gates, uint32_t blocks, const double* __restrict__ e_partials, uint32_t op_blocks, int out_width,
                       double* __restrict__ out, double* __restrict__ out_values) {
    const uint32_t pos = blockIdx.y, lane = threadIdx.x & 63;
    const long long j = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (j > out_width) return;
    const AdjEval ev = evals[pos];
    double acc = 0.0;
    if (j == out_width) {
        if (!out_values) return;
        for (uint32_t b = lane; b < op_blocks; b += 64) acc += e_partials[size_t(pos) * op_blocks + b];
        acc = wave_sum(acc);
        if (lane == 0) out_values[ev.row] = acc;
        return;
    }
    const long long first = entry_offsets[ev.row], count = entry_offsets[ev.row + 1] - first;
    if (j < count) {
        const AdjEntry en = entries[first + j];
        for (uint32_t k = 0; k < en.count; ++k) {
            const double* p = partials + (size_t(pos) * 3 * max_gates + slots[en.first + k]) * blocks;
            for (uint32_t b = lane; b < blocks; b += 64) acc += p[b];
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) out[(long long)ev.row * out_width + j] = 2.0 * acc;
}

}  // namespace

hipError_t launch_adjoint_prepare(const AdjEval* evals, int n_evals, const AdjGate* gates, uint32_t max_gates, const double* values,
                                  int64_t width, double* mats, hipStream_t stream) {
    if (n_evals <= 0 || max_gates == 0) return hipSuccess;
    const dim3 grid((max_gates + kAdjointThreads - 1) / kAdjointThreads, unsigned(n_evals));
    hipLaunchKernelGGL(adjoint_prepare_kernel, grid, dim3(kAdjointThreads), 0, stream, evals, gates, max_gates, values,
                       (long long)width, mats);
    return hipGetLastError();
}

hipError_t launch_adjoint_apply_operator(int dtype, const void* states, void* lambda, int n_qubits, int n_evals, const OperatorView& op,
                                         bool streaming, double* e_partials, hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    const dim3 grid(adjoint_op_blocks(n_qubits), unsigned(n_evals));
    const unsigned long long dim = 1ull << n_qubits;
    if (dtype == QSV_F64)
        hipLaunchKernelGGL(adjoint_apply_operator_kernel<double>, grid, dim3(kAdjointThreads), 0, stream,
                           static_cast<const acx<double>*>(states), static_cast<acx<double>*>(lambda), dim, op.diag, op.n_groups, op.groups,
                           op.term_z, op.term_coef, op.term_odd, streaming, e_partials);
    else
        hipLaunchKernelGGL(adjoint_apply_operator_kernel<float>, grid, dim3(kAdjointThreads), 0, stream,
                           static_cast<const acx<float>*>(states), static_cast<acx<float>*>(lambda), dim, op.diag, op.n_groups, op.groups,
                           op.term_z, op.term_coef, op.term_odd, streaming, e_partials);
    return hipGetLastError();
}

hipError_t launch_adjoint_run(int dtype, void* states, void* lambda, int n_qubits, int n_evals, uint32_t run, const AdjEval* evals,
                              const AdjRunDesc* runs, const AdjGate* gates, const double* mats, uint32_t max_gates, bool streaming,
                              double* partials, hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    const dim3 grid(adjoint_blocks(n_qubits), unsigned(n_evals));
    hipError_t e;
    if (dtype == QSV_F64) {
        constexpr size_t lds = run_lds_bytes<double>();
        static const hipError_t configured = hipFuncSetAttribute(reinterpret_cast<const void*>(adjoint_run_kernel<double>),
                                                                 hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if ((e = configured) != hipSuccess) return e;
        hipLaunchKernelGGL(adjoint_run_kernel<double>, grid, dim3(kAdjointThreads), lds, stream, static_cast<acx<double>*>(states),
                           static_cast<acx<double>*>(lambda), n_qubits, run, evals, runs, gates, mats, max_gates, streaming, partials);
    } else {
        constexpr size_t lds = run_lds_bytes<float>();
        static const hipError_t configured = hipFuncSetAttribute(reinterpret_cast<const void*>(adjoint_run_kernel<float>),
                                                                 hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if ((e = configured) != hipSuccess) return e;
        hipLaunchKernelGGL(adjoint_run_kernel<float>, grid, dim3(kAdjointThreads), lds, stream, static_cast<acx<float>*>(states),
                           static_cast<acx<float>*>(lambda), n_qubits, run, evals, runs, gates, mats, max_gates, streaming, partials);
    }
    return hipGetLastError();
}

hipError_t launch_adjoint_combine(const AdjEval* evals, int n_evals, const int64_t* entry_offsets, const AdjEntry* entries,
                                  const uint32_t* slots, const double* partials, uint32_t max_gates, uint32_t blocks,
                                  const double* e_partials, uint32_t op_blocks, int out_width, double* out, double* out_values,
                                  hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    const dim3 grid(unsigned((out_width + 1 + kWaves - 1) / kWaves), unsigned(n_evals));
    hipLaunchKernelGGL(adjoint_combine_kernel, grid, dim3(kAdjointThreads), 0, stream, evals,
                       reinterpret_cast<const long long*>(entry_offsets), entries, slots, partials, max_gates, blocks, e_partials,
                       op_blocks, out_width, out, out_values);
    return hipGetLastError();
}

}  // namespace qsv
