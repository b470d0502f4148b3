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

}  // namespace irn
