// The Fubini-Study metric (metric.hpp): the kernels.  metric_run_kernel sweeps psi and the living derivative
// states xi of a launch group backwards through one run of the adjoint plan and sums nothing; metric_gram_kernel forms the real
// Gram matrix of an evaluation's columns and i psi on the fp64 matrix pipe; metric_combine_kernel adds the workgroups' tiles in
// ascending order, subtracts b b^T and sums angle slots into parameters.  Every sum is fp64 whatever the state's type and is
// formed in a fixed order, so an evaluation's matrix depends on nothing but its circuit and its point.  No floating-point atomics.
#include "metric.hpp"

namespace qsv {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

template <typename real>
struct alignas(2 * sizeof(real)) mcx {  // (one access per amplitude)
    real re, im;
};

template <typename real>
__device__ __forceinline__ mcx<real> load_amp(const mcx<real>* p, bool streaming) {
    typedef real vec2 __attribute__((ext_vector_type(2)));
    const vec2 v = streaming ? __builtin_nontemporal_load(reinterpret_cast<const vec2*>(p)) : *reinterpret_cast<const vec2*>(p);
    return mcx<real>{v.x, v.y};
}
template <typename real>
__device__ __forceinline__ void store_amp(mcx<real>* p, mcx<real> a, bool streaming) {
    typedef real vec2 __attribute__((ext_vector_type(2)));
    vec2 v;
    v.x = a.re;
    v.y = a.im;
    if (streaming)
        __builtin_nontemporal_store(v, reinterpret_cast<vec2*>(p));
    else
        *reinterpret_cast<vec2*>(p) = v;
}

constexpr int kHighBits = kAdjointTileBits - kAdjointLowBits;
constexpr uint32_t kNoBirth = 0xffffffffu;

// One run of the sweep for one state of one evaluation: blockIdx.y == 0 is psi, blockIdx.y == 1 + c column c; blockIdx.z the
// evaluation's position.  A workgroup takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of its state: the tile into LDS,
// the run's gates last first, the tile back.  Tile addressing, pair loop and bank-spreading swap are adjoint_run_kernel's.  A
// column born at gate g of this run starts from PSI's tile as the run found it, takes U^dagger down to g (which makes it
// psi_(g-1), the same bits psi's own workgroup computes), then dU_g/d(slot) and U_g^dagger, then the rest of the run.  psi is read
// from the buffer the run before wrote and written to the other one, so a born column's read never meets psi's write.
template <typename real>
__global__ void __launch_bounds__(kMetricThreads)
metric_run_kernel(const mcx<real>* __restrict__ states, mcx<real>* __restrict__ scratch, unsigned long long stride, int n_qubits,
                  uint32_t run, const MetEval* __restrict__ evals, const AdjRunDesc* __restrict__ runs,
                  const AdjGate* __restrict__ gates, const MetCol* __restrict__ cols, const double* __restrict__ mats,
                  uint32_t max_gates, bool streaming) {
    __shared__ mcx<real> s_tile[1u << kAdjointTileBits];
    __shared__ uint8_t tile_qubit[kAdjointTileBits], outer_qubit[64];
    const uint32_t pos = blockIdx.z;
    const MetEval ev = evals[pos];
    if (run >= ev.n_runs) return;  // (the whole workgroup: this evaluation's sweep is over)
    const AdjRunDesc rd = runs[ev.run_base + run];
    const uint32_t n_gates = run + 1 == ev.n_runs ? ev.n_gates - rd.first_gate : rd.n_gates;
    const unsigned long long dim = 1ull << n_qubits;
    mcx<real>* const mine = scratch + (unsigned long long)pos * stride * dim;
    const mcx<real>* const psi_in = run == 0 ? states + (unsigned long long)pos * dim : mine + (unsigned long long)((run - 1) & 1u) * dim;
    const mcx<real>* src;
    mcx<real>* dst;
    uint32_t birth = kNoBirth, birth_slot = 0;
    // psi's last run leaves i psi = (-Im psi, Re psi): nothing reads psi after it but the Gram kernel, to which b = Im<psi|xi> is
    // then a row Re<i psi|xi> like every other
    const bool rotate = blockIdx.y == 0 && run + 1 == ev.n_runs;
    if (blockIdx.y == 0) {
        src = psi_in;
        dst = mine + (unsigned long long)(run & 1u) * dim;
    } else {
        const uint32_t c = blockIdx.y - 1;
        if (c >= ev.n_cols) return;
        const uint32_t slot = cols[ev.col_base + c].slot, g = slot / 3;
        if (g >= rd.first_gate + n_gates) return;  // (not yet born)
        dst = mine + (unsigned long long)(kMetricPsiBuffers + c) * dim;
        if (g >= rd.first_gate) {
            birth = g - rd.first_gate;
            birth_slot = slot - 3 * g;
            src = psi_in;
        } else {
            src = dst;
        }
    }
    const int tile_bits = n_qubits < kAdjointTileBits ? n_qubits : kAdjointTileBits;
    const uint32_t tile = 1u << tile_bits, n_pairs = tile >> 1;
    const uint32_t tid = threadIdx.x, lane = tid & 63;

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
    const int outer_bits = n_qubits - tile_bits;
    const unsigned long long n_tiles = 1ull << outer_bits;
    // the lanes of one LDS access group: 16 for 16-byte elements, 32 for 8-byte ones
    constexpr uint32_t swap_bit = sizeof(mcx<real>) == 16 ? 3 : 4;

    // (a0, a1) <- M (a0, a1) on every pair of the gate's target whose control (if any) is 1; `project`: a pair whose control is 0
    // becomes zero (the derivative's control-0 block), otherwise it is left as it is.  Ends in a barrier.
    auto apply = [&](uint32_t tpos, uint32_t cpos, const double* __restrict__ m, bool project) {
        const real m00r = real(m[0]), m00i = real(m[1]), m01r = real(m[2]), m01i = real(m[3]);
        const real m10r = real(m[4]), m10i = real(m[5]), m11r = real(m[6]), m11i = real(m[7]);
        const uint32_t tbit = 1u << tpos;
        const bool controlled = cpos != QSV_NO_CONTROL;
        const uint32_t cbit = controlled ? 1u << cpos : 0u;
        const bool swap = tpos <= swap_bit && ((lane >> swap_bit) & 1u);
        for (uint32_t p = tid; p < n_pairs; p += kMetricThreads) {
            const uint32_t i0 = ((p >> tpos) << (tpos + 1)) | (p & (tbit - 1)), i1 = i0 | tbit;
            const uint32_t ix = swap ? i1 : i0, iy = swap ? i0 : i1;
            if (controlled && !(i0 & cbit)) {
                if (project) {
                    mcx<real> zero;
                    zero.re = zero.im = real(0);
                    s_tile[ix] = zero;
                    s_tile[iy] = zero;
                }
                continue;
            }
            const mcx<real> px = s_tile[ix], py = s_tile[iy];
            mcx<real> a0, a1, b0, b1, ox, oy;  // (selected part by part: a select of whole amplitudes goes through memory)
            a0.re = swap ? py.re : px.re, a0.im = swap ? py.im : px.im;
            a1.re = swap ? px.re : py.re, a1.im = swap ? px.im : py.im;
            b0.re = m00r * a0.re - m00i * a0.im + m01r * a1.re - m01i * a1.im;
            b0.im = m00r * a0.im + m00i * a0.re + m01r * a1.im + m01i * a1.re;
            b1.re = m10r * a0.re - m10i * a0.im + m11r * a1.re - m11i * a1.im;
            b1.im = m10r * a0.im + m10i * a0.re + m11r * a1.im + m11i * a1.re;
            ox.re = swap ? b1.re : b0.re, ox.im = swap ? b1.im : b0.im;
            oy.re = swap ? b0.re : b1.re, oy.im = swap ? b0.im : b1.im;
            s_tile[ix] = ox;
            s_tile[iy] = oy;
        }
        __syncthreads();  // (the next step pairs other elements)
    };

    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        unsigned long long base = 0;
        for (int j = 0; j < outer_bits; ++j) base |= ((t >> j) & 1ull) << outer_qubit[j];
        for (uint32_t l = tid; l < tile; l += kMetricThreads) s_tile[l] = load_amp(src + (base | spread(l)), streaming);
        __syncthreads();
        for (uint32_t gl = 0; gl < n_gates; ++gl) {
            const uint32_t g = rd.first_gate + gl;
            const AdjGate* gt = gates + ev.gate_base + g;
            const uint32_t tpos = gt->tpos, cpos = gt->cpos;
            const double* m = mats + (size_t(pos) * max_gates + g) * kAdjointMatDoubles;
            apply(tpos, cpos, m, false);  // U^dagger
            if (gl == birth) {            // (the state's, so the whole workgroup's)
                apply(tpos, cpos, m + 8 * (birth_slot + 1), true);  // the tile held psi_(g-1): the column is born
                apply(tpos, cpos, m, false);
            }
        }
        for (uint32_t l = tid; l < tile; l += kMetricThreads) {
            const mcx<real> a = s_tile[l];
            mcx<real> o;
            o.re = rotate ? -a.im : a.re;
            o.im = rotate ? a.re : a.im;
            store_amp(dst + (base | spread(l)), o, streaming);
        }
        __syncthreads();  // (the next tile's loads overwrite what these stores read)
    }
}

constexpr uint32_t kRow = 66;  // doubles per panel row: lanes m = 0 .. 15 read 8-byte words 4 m + 2 k apart, every bank once
constexpr uint32_t kPanel = (kMetBlock + 1) * kRow;  // (row 16: the spare row)

// the four registers of an accumulator to their places of a 16 x 16 tile: column = lane & 15, row = (lane >> 4) + 4 * register
__device__ __forceinline__ void store_tile(double* __restrict__ out, v4d acc, uint32_t lane) {
    out[((lane >> 4) + 0) * 16 + (lane & 15)] = acc.x;
    out[((lane >> 4) + 4) * 16 + (lane & 15)] = acc.y;
    out[((lane >> 4) + 8) * 16 + (lane & 15)] = acc.z;
    out[((lane >> 4) + 12) * 16 + (lane & 15)] = acc.w;
}

// grid: (workgroups, pairs of blocks, evaluations); a workgroup is one wave.  It takes one pair (rb <= cb) of blocks of 16 of the
// evaluation's vectors -- its columns, then i psi as psi's last run left it -- and 64 consecutive amplitudes at a time, writes them
// to LDS panels [vector][amplitude] (overlap_panels_kernel's layout) and accumulates sum (a_re b_re + a_im b_im): the matrix
// instruction sums over four amplitudes, real and imaginary parts as separate steps.
template <typename real>
__global__ void __launch_bounds__(64)
metric_gram_kernel(const mcx<real>* __restrict__ scratch, unsigned long long stride, unsigned long long dim,
                   const MetEval* __restrict__ evals, uint32_t max_pairs, double* __restrict__ partials) {
    // (row 16 of a panel is never read: what belongs to no vector of the tile is written there, so the rows of unused vectors, and
    // the amplitudes past 2^n of a register below six qubits, keep the zeros they are given here)
    __shared__ double a_re[kPanel], a_im[kPanel], b_re[kPanel], b_im[kPanel];
    const uint32_t lane = threadIdx.x, pair = blockIdx.y, pos = blockIdx.z;
    const MetEval ev = evals[pos];
    if (ev.n_cols == 0) return;
    const uint32_t n_vec = ev.n_cols + 1, nb = (n_vec + kMetBlock - 1) / kMetBlock;
    if (pair >= nb * (nb + 1) / 2) return;
    uint32_t cb = 0;
    while ((cb + 1) * (cb + 2) / 2 <= pair) ++cb;
    const uint32_t rb = pair - cb * (cb + 1) / 2;
    for (uint32_t j = 0; j <= kMetBlock; ++j)
        a_re[j * kRow + lane] = a_im[j * kRow + lane] = b_re[j * kRow + lane] = b_im[j * kRow + lane] = 0.0;
    // lane l supplies the operand element (vector l & 15, amplitude 4 s + (l >> 4) of the 64) of both sides at step s
    const uint32_t at = (lane & 15) * kRow + (lane >> 4);
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    const uint32_t n_r = min(kMetBlock, n_vec - rb * kMetBlock), n_c = min(kMetBlock, n_vec - cb * kMetBlock);
    const bool live = lane < dim;
    const uint32_t spare = kMetBlock * kRow + lane, mine = live ? lane : 0u;
    const uint32_t psi_state = (ev.n_runs - 1) & 1u;  // the buffer psi's last run wrote: i psi
    // Per row j, fixed before the walk: where the lane's amplitude of chunk 0 is and where it goes in the panel -- an unused row reads the block's first vector, which is there, a dead lane reads amplitude 0, and both write
    // row 16.  j is never a run-time index.
    unsigned long long row_at[kMetBlock], col_at[kMetBlock];
    uint32_t row_to[kMetBlock], col_to[kMetBlock];
    const unsigned long long first = (unsigned long long)pos * stride;
#pragma unroll
    for (uint32_t j = 0; j < kMetBlock; ++j) {
        const uint32_t vr = rb * kMetBlock + (j < n_r ? j : 0u), vc = cb * kMetBlock + (j < n_c ? j : 0u);
        // (the state numbers go to vector registers at once: sixteen products kept in scalar registers are more than there are)
        uint32_t sr = vr == ev.n_cols ? psi_state : kMetricPsiBuffers + vr, sc = vc == ev.n_cols ? psi_state : kMetricPsiBuffers + vc;
        asm volatile("" : "+v"(sr), "+v"(sc));
        row_at[j] = (first + sr) * dim + mine;
        col_at[j] = (first + sc) * dim + mine;
        row_to[j] = live && j < n_r ? j * kRow + lane : spare;
        col_to[j] = live && j < n_c ? j * kRow + lane : spare;
    }
    const unsigned long long chunks = (dim + 63) / 64;
    for (unsigned long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
#pragma unroll
        for (uint32_t j = 0; j < kMetBlock; ++j) {
            const mcx<real> a = scratch[row_at[j] + chunk * 64];
            a_re[row_to[j]] = double(a.re);
            a_im[row_to[j]] = double(a.im);
        }
#pragma unroll
        for (uint32_t j = 0; j < kMetBlock; ++j) {
            const mcx<real> b = scratch[col_at[j] + chunk * 64];
            b_re[col_to[j]] = double(b.re);
            b_im[col_to[j]] = double(b.im);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const double ar = a_re[at + 4 * s], ai = a_im[at + 4 * s];
            const double br = b_re[at + 4 * s], bi = b_im[at + 4 * s];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bi, acc, 0, 0, 0);
        }
        __syncthreads();  // (the next chunk's panels go into the same LDS)
    }
    store_tile(partials + ((size_t(pos) * max_pairs + pair) * gridDim.x + blockIdx.x) * kMetTile, acc, lane);
}

// One thread per entry (i <= j) of an evaluation's matrix; it writes the entry and its mirror image.
__global__ void __launch_bounds__(kMetricThreads)
metric_combine_kernel(const MetEval* __restrict__ evals, const MetEntry* __restrict__ entries, const uint32_t* __restrict__ entry_cols,
                      const double* __restrict__ partials, uint32_t max_pairs, uint32_t blocks, uint32_t width, double* __restrict__ out) {
    const uint32_t pos = blockIdx.y;
    const unsigned long long idx = (unsigned long long)blockIdx.x * kMetricThreads + threadIdx.x;
    if (idx >= (unsigned long long)width * width) return;
    const uint32_t i = uint32_t(idx / width), j = uint32_t(idx % width);
    if (i > j) return;
    const MetEval ev = evals[pos];
    double* o = out + (size_t(ev.row) * width) * width;
    double total = 0.0;
    if (j < ev.n_entries && ev.n_cols > 0) {
        const double* mine = partials + size_t(pos) * max_pairs * blocks * kMetTile;
        // the sum over workgroups, ascending, of entry (r, c) of the Gram matrix, read from its upper triangle
        auto gram = [&](uint32_t r, uint32_t c) {
            if (r > c) {
                const uint32_t t = r;
                r = c;
                c = t;
            }
            const uint32_t rb = r >> 4, cb = c >> 4;
            const double* p = mine + size_t(cb * (cb + 1) / 2 + rb) * blocks * kMetTile + (r & 15) * 16 + (c & 15);
            double sum = 0.0;
            for (uint32_t w = 0; w < blocks; ++w) sum += p[size_t(w) * kMetTile];
            return sum;
        };
        // (the entry whose first column was born later -- the earlier gate -- is the outer loop whichever of i and j it is: the
        // same order of the same terms for (i, j) of any wrt list)
        MetEntry ea = entries[ev.entry_base + i], eb = entries[ev.entry_base + j];
        if (ea.count && eb.count && entry_cols[ea.first] < entry_cols[eb.first]) {
            const MetEntry t = ea;
            ea = eb;
            eb = t;
        }
        for (uint32_t x = 0; x < ea.count; ++x) {
            const uint32_t a = entry_cols[ea.first + x];
            const double ba = gram(a, ev.n_cols);
            for (uint32_t y = 0; y < eb.count; ++y) {
                const uint32_t b = entry_cols[eb.first + y];
                total += gram(a, b) - ba * gram(b, ev.n_cols);
            }
        }
    }
    o[size_t(i) * width + j] = total;
    o[size_t(j) * width + i] = total;
}

template <typename real>
void launch_run(const void* states, void* scratch, uint64_t stride, int n_qubits, int n_evals, uint32_t max_cols, uint32_t run,
                const MetEval* evals, const AdjRunDesc* runs, const AdjGate* gates, const MetCol* cols, const double* mats,
                uint32_t max_gates, bool streaming, hipStream_t stream) {
    const dim3 grid(metric_blocks(n_qubits), 1 + max_cols, unsigned(n_evals));
    hipLaunchKernelGGL(metric_run_kernel<real>, grid, dim3(kMetricThreads), 0, stream, static_cast<const mcx<real>*>(states),
                       static_cast<mcx<real>*>(scratch), (unsigned long long)stride, n_qubits, run, evals, runs, gates, cols, mats, max_gates,
                       streaming);
}

}  // namespace

hipError_t launch_metric_run(int dtype, const void* states, void* scratch, uint64_t stride, int n_qubits, int n_evals, uint32_t max_cols,
                             uint32_t run, const MetEval* evals, const AdjRunDesc* runs, const AdjGate* gates, const MetCol* cols,
                             const double* mats, uint32_t max_gates, bool streaming, hipStream_t stream) {
    if (n_evals <= 0) return hipSuccess;
    if (dtype == QSV_F64)
        launch_run<double>(states, scratch, stride, n_qubits, n_evals, max_cols, run, evals, runs, gates, cols, mats, max_gates, streaming, stream);
    else
        launch_run<float>(states, scratch, stride, n_qubits, n_evals, max_cols, run, evals, runs, gates, cols, mats, max_gates, streaming, stream);
    return hipGetLastError();
}

hipError_t launch_metric_gram(int dtype, const void* scratch, uint64_t stride, int n_qubits, int n_evals, uint32_t max_cols,
                              const MetEval* evals, double* partials, hipStream_t stream) {
    if (n_evals <= 0 || max_cols == 0) return hipSuccess;
    const uint32_t max_pairs = metric_pairs(max_cols);
    const dim3 grid(metric_gram_blocks(n_qubits), max_pairs, unsigned(n_evals));
    const unsigned long long dim = 1ull << n_qubits;
    if (dtype == QSV_F64)
        hipLaunchKernelGGL(metric_gram_kernel<double>, grid, dim3(64), 0, stream, static_cast<const mcx<double>*>(scratch),
                           (unsigned long long)stride, dim, evals, max_pairs, partials);
    else
        hipLaunchKernelGGL(metric_gram_kernel<float>, grid, dim3(64), 0, stream, static_cast<const mcx<float>*>(scratch),
                           (unsigned long long)stride, dim, evals, max_pairs, partials);
    return hipGetLastError();
}

hipError_t launch_metric_combine(const MetEval* evals, int n_evals, const MetEntry* entries, const uint32_t* entry_cols,
                                 const double* partials, uint32_t max_pairs, uint32_t blocks, int out_width, double* out,
                                 hipStream_t stream) {
    if (n_evals <= 0 || out_width <= 0) return hipSuccess;
    const uint64_t cells = uint64_t(out_width) * uint64_t(out_width);
    const dim3 grid(unsigned((cells + kMetricThreads - 1) / kMetricThreads), unsigned(n_evals));
    hipLaunchKernelGGL(metric_combine_kernel, grid, dim3(kMetricThreads), 0, stream, evals, entries, entry_cols, partials, max_pairs, blocks,
                       uint32_t(out_width), out);
    return hipGetLastError();
}

}  // namespace qsv
