// Host-side launch plumbing shared by linear.hip, conv.hip and conv1.hip: tile dispatch, grid size, dynamic-LDS opt-in.
#pragma once
#include <type_traits>
#include "common.h"

// Turns the run-time (mi, wn) of gemm::choose_tile (each 1 or 2) into template arguments: f(MI, WN) gets two
// std::integral_constant<int, .> values.  Whatever f instantiates from them is instantiated for all four pairs; a caller that
// must not take one of them maps it onto another inside f (the fp16 linear path does).
template <class F>
void dispatch_tile(int mi, int wn, F&& f) {
    using one = std::integral_constant<int, 1>;
    using two = std::integral_constant<int, 2>;
    if (wn == 2) { if (mi == 2) f(two{}, two{}); else f(one{}, two{}); }
    else         { if (mi == 2) f(two{}, one{}); else f(one{}, one{}); }
}

// The output tiles of an m x n problem cut into Cfg::BM x Cfg::BN blocks, written to p.tiles_m / p.tiles_n (the kernels find
// their tile from them); returns their product, the 1-D grid.
template <class Cfg, class Args>
int set_tiles(Args& p, int n) {
    p.tiles_m = cdiv(p.m, Cfg::BM);
    p.tiles_n = cdiv(n, Cfg::BN);
    return p.tiles_m * p.tiles_n;
}

// More than 64 KB of dynamic LDS needs an opt-in, once per kernel and process.  The kernel is a template argument so that
// every kernel gets a flag of its own (two kernels of one signature would share the flag of a function parameter).
template <auto Kernel>
void opt_in_lds(size_t bytes) {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        attr_set = true;
    }
}
