// Compile-time path tables and the straight-line path maximum shared by the kernels that walk an LDS edge tile with
// its radial halo (affinity.hip: the walk's weight table; aff_loss.hip: the fused training loss).
#pragma once
#include <utility>

#include "kernels.hpp"

namespace irn {

constexpr int AFF_TH = kAffTileH;   // source rows per workgroup
constexpr int AFF_TW = kAffTileW;   // source cols per workgroup (one wave covers two rows)

__device__ __forceinline__ float max3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

template <int R>
struct Paths {
    static constexpr int kMaxDirs = 2 * R * R, kMaxCells = 32 * R * R;
    int n_dirs = 0, n_cells = 0;
    signed char dy[kMaxDirs] = {}, dx[kMaxDirs] = {};
    short start[kMaxDirs + 1] = {};
    signed char cy[kMaxCells] = {}, cx[kMaxCells] = {};
    constexpr void add(int y, int x) {
        // thick segment (0,0) -> (y,x): lattice points of the bounding box with (y*px - x*py)^2 < y^2 + x^2
        // (misc/indexing.py:37-46); the max over a path does not depend on the order of its cells
        dy[n_dirs] = (signed char)y;
        dx[n_dirs] = (signed char)x;
        const int lsq = y * y + x * x;
        const int x_lo = x < 0 ? x : 0, x_hi = x < 0 ? 0 : x;
        for (int py = 0; py <= y; ++py)
            for (int px = x_lo; px <= x_hi; ++px) {
                const int cross = y * px - x * py;
                if (cross * cross < lsq) {
                    cy[n_cells] = (signed char)py;
                    cx[n_cells] = (signed char)px;
                    ++n_cells;
                }
            }
        start[++n_dirs] = (short)n_cells;
    }
    constexpr Paths() {
        // raster order of the directions = discovery order of misc/indexing.py:24-30 (path table order 1)
        for (int x = 1; x < R; ++x) add(0, x);
        for (int y = 1; y < R; ++y)
            for (int x = -R + 1; x < R; ++x)
                if (x * x + y * y < R * R) add(y, x);
    }
};
template <int R>
inline constexpr Paths<R> kPaths{};

template <int... Is, typename F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, Is...>, F &&f) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
    static_for_impl(std::make_integer_sequence<int, N>{}, f);
}

template <int R, int D>
__device__ __forceinline__ float path_max(const float *tb) {
    constexpr int LW = AFF_TW + 2 * (R - 1), HALO = R - 1;
    constexpr int k0 = kPaths<R>.start[D], n = kPaths<R>.start[D + 1] - k0;
    constexpr auto off = [](int k) constexpr { return kPaths<R>.cy[k] * LW + kPaths<R>.cx[k] + HALO; };
    float m = tb[off(k0)];
    static_for<(n - 1) / 2>([&](auto ik) __attribute__((always_inline)) {
        constexpr int k = k0 + 1 + 2 * decltype(ik)::value;
        m = max3(m, tb[off(k)], tb[off(k + 1)]);
    });
    if constexpr ((n - 1) % 2 == 1) {
        const float v = tb[off(k0 + n - 1)];
        m = max3(m, v, v);
    }
    return m;
}

// ------------------------------------------------------------------------------------------------
// P horizontally adjacent pixels per lane (affinity.hip: affinity_wide_kernel).  The P floats a lane needs of path
// cell (cy, cx) start at column x0 + cx + HALO of the staged tile; with x0 and the row stride multiples of P their
// alignment is (cx + HALO) mod P, a constant of the cell.  The tile is staged P times, copy s shifted left by s floats,
// so that cell is one aligned 4P-byte read of copy (cx + HALO) mod P with its offset as the instruction's immediate.
// ------------------------------------------------------------------------------------------------
template <int R, int P>
struct WideTile {
    static_assert(P == 2, "8-byte LDS reads");
    // 16 lanes x 16 rows: 32 columns keep the ragged grids' loss where the 8 x 32 tile had it (94 -> 96, 125 -> 128)
    static constexpr int TW = 32, TH = 16;
    static constexpr int LANES_X = TW / P, HALO = R - 1, LW = TW + 2 * HALO, LH = TH + HALO;
    // Row stride in floats.  ds_read_b64 is served 32 lanes at a time over 64 banks: 16 lanes of one row read 32
    // consecutive words, the other 16 the same words of the next row, so the stride is 32 mod 64 and the two rows
    // take the two halves of the banks.
    static constexpr int STRIDE = (LW + 31) / 64 * 64 + 32;
    static constexpr int COPY = LH * STRIDE;                    // floats per shifted copy
    static_assert(TW % P == 0 && LANES_X * TH == 256, "one lane per P pixels, 256 lanes");
    static_assert(STRIDE >= LW && STRIDE % P == 0 && COPY % P == 0, "aligned rows and copies");
    static_assert(STRIDE % 64 == 32 && LANES_X * P == 32, "two rows of a ds_read_b64 group on disjoint banks");
    static_assert(P * COPY * 4 <= 65536, "LDS offsets are 16-bit immediates");
};

template <int P>
using floatP = float __attribute__((ext_vector_type(P)));

// N aligned 4P-byte reads of the LDS at byte address `a` plus the immediates O + 0 .. N-1, and the wait for them, as one
// instruction group.  Written out because the compiler pairs plain 8-byte reads into ds_read2_b64, which the LDS serves
// at half the rate of two ds_read_b64; the other waves of the SIMD cover the wait.
#define IRN_DS_RD(i) IRN_DS_OP " %" #i ", %[a] offset:%[o" #i "]\n\t"
#define IRN_DS_READS(P_)                                                                                               \
    template <int O0, int O1, int O2, int O3, int O4, int O5, int O6, int O7>                                          \
    __device__ __forceinline__ void lds_read8(unsigned a, floatP<P_> *v) {                                             \
        asm volatile(IRN_DS_RD(0) IRN_DS_RD(1) IRN_DS_RD(2) IRN_DS_RD(3) IRN_DS_RD(4) IRN_DS_RD(5) IRN_DS_RD(6)        \
                     IRN_DS_RD(7) "s_waitcnt lgkmcnt(0)"                                                               \
                     : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]),      \
                       "=&v"(v[7])                                                                                     \
                     : [a] "v"(a), [o0] "n"(O0), [o1] "n"(O1), [o2] "n"(O2), [o3] "n"(O3), [o4] "n"(O4), [o5] "n"(O5), \
                       [o6] "n"(O6), [o7] "n"(O7));                                                                    \
    }                                                                                                                  \
    template <int O0, int O1, int O2, int O3>                                                                          \
    __device__ __forceinline__ void lds_read4(unsigned a, floatP<P_> *v) {                                             \
        asm volatile(IRN_DS_RD(0) IRN_DS_RD(1) IRN_DS_RD(2) IRN_DS_RD(3) "s_waitcnt lgkmcnt(0)"                        \
                     : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])                                              \
                     : [a] "v"(a), [o0] "n"(O0), [o1] "n"(O1), [o2] "n"(O2), [o3] "n"(O3));                            \
    }                                                                                                                  \
    template <int O0, int O1>                                                                                          \
    __device__ __forceinline__ void lds_read2(unsigned a, floatP<P_> *v) {                                             \
        asm volatile(IRN_DS_RD(0) IRN_DS_RD(1) "s_waitcnt lgkmcnt(0)"                                                  \
                     : "=&v"(v[0]), "=&v"(v[1])                                                                        \
                     : [a] "v"(a), [o0] "n"(O0), [o1] "n"(O1));                                                        \
    }                                                                                                                  \
    template <int O0>                                                                                                  \
    __device__ __forceinline__ void lds_read1(unsigned a, floatP<P_> *v) {                                             \
        asm volatile(IRN_DS_RD(0) "s_waitcnt lgkmcnt(0)" : "=&v"(v[0]) : [a] "v"(a), [o0] "n"(O0));                    \
    }
#define IRN_DS_OP "ds_read_b64"
IRN_DS_READS(2)
#undef IRN_DS_OP
#undef IRN_DS_READS
#undef IRN_DS_RD

// Maxima of direction D for the P pixels whose first one has its tile origin at LDS byte address `a` (copy 0, a multiple
// of 4P): per pixel the same v_max3_f32 chain over the same cells in the same order as path_max.
template <int R, int P, int D>
__device__ __forceinline__ floatP<P> path_max_wide(unsigned a) {
    using T = WideTile<R, P>;
    constexpr int k0 = kPaths<R>.start[D], n = kPaths<R>.start[D + 1] - k0;
    constexpr auto off = [](int i) constexpr {      // byte offset of cell i of the path
        const int c = kPaths<R>.cx[k0 + i] + T::HALO, s = c % P;
        return 4 * (s * T::COPY + kPaths<R>.cy[k0 + i] * T::STRIDE + c - s);
    };
    floatP<P> v[n];
    static_for<n / 8>([&](auto ib) __attribute__((always_inline)) {
        constexpr int i = 8 * decltype(ib)::value;
        lds_read8<off(i), off(i + 1), off(i + 2), off(i + 3), off(i + 4), off(i + 5), off(i + 6), off(i + 7)>(a, v + i);
    });
    constexpr int i4 = n / 8 * 8, i2 = i4 + (n & 4), i1 = i2 + (n & 2);
    if constexpr (n & 4) lds_read4<off(i4), off(i4 + 1), off(i4 + 2), off(i4 + 3)>(a, v + i4);
    if constexpr (n & 2) lds_read2<off(i2), off(i2 + 1)>(a, v + i2);
    if constexpr (n & 1) lds_read1<off(i1)>(a, v + i1);
    static_assert(off(0) % (4 * P) == 0 && off(n - 1) % (4 * P) == 0 && off(n - 1) + 4 * P <= 4 * P * T::COPY, "aligned, inside");
    floatP<P> m = v[0];
    static_for<(n - 1) / 2>([&](auto ik) __attribute__((always_inline)) {
        constexpr int k = 1 + 2 * decltype(ik)::value;
        static_for<P>([&](auto ip) __attribute__((always_inline)) {
            constexpr int p = decltype(ip)::value;
            m[p] = max3(m[p], v[k][p], v[k + 1][p]);
        });
    });
    if constexpr ((n - 1) % 2 == 1) {
        static_for<P>([&](auto ip) __attribute__((always_inline)) {
            constexpr int p = decltype(ip)::value;
            m[p] = max3(m[p], v[n - 1][p], v[n - 1][p]);
        });
    }
    return m;
}

}  // namespace irn
