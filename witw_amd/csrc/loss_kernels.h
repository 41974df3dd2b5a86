// The loss kernels that cvig_fov (Term = FovTerm) and cvig_baseline (Term = BaselineTerm) share, on a COLUMN SLAB of the global
// batch: this rank holds D [B,b] = the distances of all B rows to the columns [col0, col0+b) of the global matrix (local column j is
// global column c = col0 + j), and diag [B], the global diagonal. l = Term::value, l' = Term::deriv; with Term::skip_diag the sums
// leave out the entries i == c.
//
//   exhaustive   part[i]   = sum_j l(diag[c] - D[i][j]) + l(diag[i] - D[i][j])
//                rowsig[i] = sum_j l'(diag[i] - D[i][j])   (this rank's columns only: the caller sums it over the ranks)
//                colsig[j] = sum_i l'(diag[c] - D[i][j])   (complete)
//                G[i][j]   = sc (-l'(diag[c] - D[i][j]) - l'(diag[i] - D[i][j]) + [i == c] (colsig[j] + rowsig[i]))
//   batch-hard   rv, ri / cv, ci = min and argmin of the global rows / of the slab's columns, the diagonal masked (loss_hard.hip)
//                out = (sum_j l(d_c - rv[c]) + l(d_c - cv[j])) / norm
//                the pair list of hard_pairs_kernel
//
// Every sum runs in a fixed order (a thread's strided partial, then block_sum_256) and nothing is accumulated with atomics: the same
// call gives the same bits.
#pragma once
#include "loss_terms.h"

namespace {

// one block per row i of the slab
template <class Term>
__global__ __launch_bounds__(256) void slab_partials_kernel(const float* __restrict__ D, const float* __restrict__ diag,
                                                             float* __restrict__ part, int b, int col0, Term term) {
    __shared__ float sh[4];
    const int i = blockIdx.x;
    const float dii = diag[i];
    float s = 0.f;
    for (int j = threadIdx.x; j < b; j += 256) {
        if (Term::skip_diag && col0 + j == i) continue;
        const float d = D[(size_t)i * b + j];
        s += term.value(diag[col0 + j] - d);
        s += term.value(dii - d);
    }
    const float tot = block_sum_256(s, sh);
    if (threadIdx.x == 0) part[i] = tot;
}

// blocks [0,B): rowsig[i] over this slab's columns; blocks [B,B+b): colsig[j] over all rows
template <class Term>
__global__ __launch_bounds__(256) void slab_sig_kernel(const float* __restrict__ D, const float* __restrict__ diag,
                                                        float* __restrict__ rowsig, float* __restrict__ colsig, int B, int b, int col0,
                                                        Term term) {
    __shared__ float sh[4];
    const bool is_col = blockIdx.x >= (unsigned)B;
    const int m = is_col ? blockIdx.x - B : blockIdx.x;
    const int own = is_col ? col0 + m : m;               // the global index whose diagonal entry is the positive distance
    const float dm = diag[own];
    const int cnt = is_col ? B : b;
    float s = 0.f;
    for (int t = threadIdx.x; t < cnt; t += 256) {
        if (Term::skip_diag && (is_col ? t : col0 + t) == own) continue;
        const float d = is_col ? D[(size_t)t * b + m] : D[(size_t)m * b + t];
        s += term.deriv(dm - d);
    }
    const float tot = block_sum_256(s, sh);
    if (threadIdx.x == 0) (is_col ? colsig : rowsig)[m] = tot;
}

// rowsig = the row sums over ALL columns (summed over the ranks by the caller); gloss = the gradient of the GLOBAL loss
template <class Term>
__global__ void slab_bwd_kernel(const float* __restrict__ D, const float* __restrict__ diag, const float* __restrict__ rowsig,
                                const float* __restrict__ colsig, const float* __restrict__ gloss, float* __restrict__ G, int B, int b,
                                int col0, Term term) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * b) return;
    const int i = idx / b, j = idx - (size_t)i * b;
    const bool on_diag = i == col0 + j;
    float g;
    if (Term::skip_diag && on_diag) {
        g = colsig[j] + rowsig[i];
    } else {
        const float d = D[idx];
        g = -term.deriv(diag[col0 + j] - d) - term.deriv(diag[i] - d);
        if (on_diag) g += colsig[j] + rowsig[i];
    }
    G[idx] = g * term.scale(gloss[0], 2.f * B * (B - 1));
}

// One workgroup. norm = 1: the rank's partial; 2B: the loss of the full form.
template <class Term>
__global__ __launch_bounds__(256) void hard_loss_kernel(const float* __restrict__ D, const float* __restrict__ rv,
                                                         const float* __restrict__ cv, float* __restrict__ out, int b, int col0,
                                                         Term term, float norm) {
    __shared__ float sh[4];
    float s = 0.f;
    for (int j = threadIdx.x; j < b; j += 256) {
        const int c = col0 + j;
        const float d = D[(size_t)c * b + j];
        s += term.hard_value(d - rv[c]);
        s += term.hard_value(d - cv[j]);
    }
    const float tot = block_sum_256(s, sh);
    if (threadIdx.x == 0) out[0] = tot / norm;
}

// Pair list of the gradient restricted to the slab's columns (s = local column), w_r[i] = sc l'(d_i - rv_i), w_c[j] = sc l'(d_c - cv_j),
// sc = Term::scale(gloss, 2B). n = 2b + B entries:
//   [0, b)        (c, j)            +w_r[c] + w_c[j]      the diagonal of column j, c = col0 + j
//   [b, 2b)       (ci[j], j)        -w_c[j]
//   [2b, 2b+B)    (i, ri[i] - col0) -w_r[i] when the slab holds column ri[i], else (-1, -1, 0) (skipped by the pair-list backwards)
template <class Term>
__global__ __launch_bounds__(256) void hard_pairs_kernel(const float* __restrict__ diag, const float* __restrict__ rv,
                                                          const long long* __restrict__ ri, const float* __restrict__ cv,
                                                          const long long* __restrict__ ci, const float* __restrict__ gloss,
                                                          int* __restrict__ po, int* __restrict__ ps, float* __restrict__ pw, int B, int b,
                                                          int col0, Term term) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * b + B) return;
    const float sc = term.scale(gloss[0], 2.f * B);
    int o = -1, s = -1;
    float w = 0.f;
    if (t < b) {
        const int c = col0 + t;
        o = c;
        s = t;
        w = sc * term.deriv(diag[c] - rv[c]) + sc * term.deriv(diag[c] - cv[t]);
    } else if (t < 2 * b) {
        const int j = t - b;
        const long long r = ci[j];
        if (r >= 0 && r < B) {
            o = (int)r;
            s = j;
            w = -(sc * term.deriv(diag[col0 + j] - cv[j]));
        }
    } else {
        const int i = t - 2 * b;
        const long long c = ri[i];
        if (c >= col0 && c < col0 + b) {
            o = i;
            s = (int)(c - col0);
            w = -(sc * term.deriv(diag[i] - rv[i]));
        }
    }
    po[t] = o;
    ps[t] = s;
    pw[t] = w;
}

}  // namespace
