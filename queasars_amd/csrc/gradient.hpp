// Parameter-shift gradients (qsv.h: qsv_gradient_describe, qsv_gradient_circuits, qsv_gradient_device): the shift plan of a
// circuit, and the two kernels around the shifted evaluations -- the expansion of base rows into shifted rows in front of them
// and the combination of their values into gradient entries behind them.  And what consumes them on the device: the Adam step.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/qsv.h"

namespace qsv {

// The shifts and coefficients of the two rules, as qsv.h documents them (doubles; every one is formed exactly like this).
inline double grad_shift1() { return M_PI_2; }
inline double grad_shift3() { return 3.0 * M_PI_2; }
inline double grad_cp() { return (std::sqrt(2.0) + 1.0) / (4.0 * std::sqrt(2.0)); }
inline double grad_cm() { return (std::sqrt(2.0) - 1.0) / (4.0 * std::sqrt(2.0)); }

// Shifted evaluations a scratch matrix holds at most, by default (qsv_set_option "gradient_chunk"): at the 240 parameters of
// a four-layer circuit on 20 qubits 16 MB of rows, about two milliseconds of evaluation per chunk.
constexpr int kGradientChunkRows = 8192;

// out[p] = evaluations the derivative by parameter p takes: 0 (no gate reads it), 2 (an angle of u, phi or lambda of cu3),
// 4 (theta of cu3), -1 (more than one angle slot reads it).  id gates read nothing.  Returns the number of parameters with -1.
int gradient_plan(int n_ops, const qsv_op* ops, int n_params, int32_t* out);

// One shifted evaluation: row `base_row` of the base matrix with entry `param` replaced by (entry + shift).  16 bytes.
struct GradRow {
    int32_t base_row;
    int32_t param;
    double shift;  // signed
};

// One gradient entry: its n_terms (0, 2 or 4) values start at values[first_value], in the order +s1, -s1, +s3, -s3.
struct GradEntry {
    int64_t first_value;
    int32_t n_terms;
    int32_t reserved;
};

// out[r][c] for r < n_rows, c < out_width (even; `out` 16-byte aligned): base[rows[r].base_row * base_stride + c] for
// c < base_width, 0 beyond, and that entry + rows[r].shift at c == rows[r].param.  One wave per row and block of 128 columns,
// one 16-byte store per thread.
hipError_t launch_gradient_expand(const double* base, int64_t base_stride, int base_width, const GradRow* rows, int64_t n_rows,
                                  double* out, int out_width, hipStream_t stream);

// out[e * out_width + j] for e < n_evals, j < out_width: entry entries[offsets[e] + j] combined from its values while
// j < offsets[e + 1] - offsets[e], 0 beyond.  Two terms: 0.5 * (v0 - v1); four: cp * (v0 - v1) - cm * (v2 - v3); every
// product and difference rounded on its own.
hipError_t launch_gradient_combine(const double* values, const GradEntry* entries, const int64_t* offsets, int64_t n_evals,
                                   int out_width, double cp, double cm, double* out, hipStream_t stream);

// qsv_adam_step (qsv.h): one wave per run -- lanes stride over the run's variables, and the squared norm of the update is summed in
// ascending j, one addition at a time --, one launch per iteration.  The arguments are the public struct's.
hipError_t launch_adam_step(const qsv_adam_step_args& args, hipStream_t stream);

}  // namespace qsv
