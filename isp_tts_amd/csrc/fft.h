// Radix-4 Stockham FFT in LDS, shared by features.hip (STFT, YIN autocorrelation) and the 1024 / 256 tile of stft_tile.h (the
// ISTFT head, the denoiser, Griffin-Lim).
//
// Complex values are float2 (re, im).  `tw` is an LDS table of kTw twiddles W_kTw^m = exp(-2 pi i m / kTw), m < kTw, made in
// float64 and rounded once (data.features.twiddles() holds kTw = 2048; W_1024^m is its entry 2m, the same fp32 value).  An
// N-point transform needs N <= kTw.  kT threads of one workgroup run one transform (lt = 0 .. kT - 1); several transforms may
// run side by side in one workgroup, because every barrier here is a workgroup barrier that all of them reach together.
#pragma once
#include "common.h"

typedef float2 cf;

__device__ __forceinline__ cf cadd(cf a, cf b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cf csub(cf a, cf b) { return make_float2(a.x - b.x, a.y - b.y); }
template <bool kInv>
__device__ __forceinline__ cf ctw(cf a, cf w) {      // a * w, or a * conj(w) for the inverse transform
    return kInv ? make_float2(a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y)
                : make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

// One Stockham autosort pass of an N-point complex DFT, in -> out; Ns = the product of the radices before it.
template <int R, bool kInv, int kT, int kTw>
__device__ __forceinline__ void fft_pass(const cf* in, cf* out, int N, int Ns, int lt, const cf* tw) {
    const int q = N / R;
    for (int j = lt; j < q; j += kT) {
        const int k = j & (Ns - 1);
        const int s = (kTw / (R * Ns)) * k;
        const int idx = (j - k) * R + k;
        if (R == 4) {
            const cf a0 = in[j], a1 = ctw<kInv>(in[j + q], tw[s]), a2 = ctw<kInv>(in[j + 2 * q], tw[2 * s]),
                     a3 = ctw<kInv>(in[j + 3 * q], tw[3 * s]);
            const cf t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), d = csub(a1, a3);
            const cf t3 = kInv ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);     // d * (+-i)
            out[idx] = cadd(t0, t2);
            out[idx + Ns] = cadd(t1, t3);
            out[idx + 2 * Ns] = csub(t0, t2);
            out[idx + 3 * Ns] = csub(t1, t3);
        } else {
            const cf a0 = in[j], a1 = ctw<kInv>(in[j + q], tw[s]);
            out[idx] = cadd(a0, a1);
            out[idx + Ns] = csub(a0, a1);
        }
    }
}

// N-point complex FFT (N = 512 or 1024) of a (ping) -> b (pong): an odd number of passes, so the result is in b.  The
// inverse is unnormalised (sum_k Z_k exp(+2 pi i k n / N)).
template <bool kInv, int kT, int kTw>
__device__ __forceinline__ void fft(cf* a, cf* b, int N, int lt, const cf* tw) {
    fft_pass<4, kInv, kT, kTw>(a, b, N, 1, lt, tw);
    __syncthreads();
    fft_pass<4, kInv, kT, kTw>(b, a, N, 4, lt, tw);
    __syncthreads();
    fft_pass<4, kInv, kT, kTw>(a, b, N, 16, lt, tw);
    __syncthreads();
    fft_pass<4, kInv, kT, kTw>(b, a, N, 64, lt, tw);
    __syncthreads();
    if (N == 1024)
        fft_pass<4, kInv, kT, kTw>(a, b, N, 256, lt, tw);
    else
        fft_pass<2, kInv, kT, kTw>(a, b, N, 256, lt, tw);
    __syncthreads();
}

// X_k (k <= n2) of a real sequence x of 2 n2 points, from Z = DFT_{n2}(x[2n] + i x[2n+1]) (the half-length split);
// w = W_{2 n2}^k
__device__ __forceinline__ cf real_split(const cf* Z, int k, int n2, cf w) {
    const cf zk = Z[k & (n2 - 1)], zm = Z[(n2 - k) & (n2 - 1)];
    const cf e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));      // (Z_k + conj Z_{-k}) / 2
    const cf dd = make_float2(zk.x - zm.x, zk.y + zm.y);                       // Z_k - conj Z_{-k}
    const cf o = make_float2(0.5f * dd.y, -0.5f * dd.x);                       // dd / 2i
    return cadd(e, ctw<false>(o, w));
}
