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

// Record of the last size-dependent launch of the calling host thread (capi.hip keeps it next to the error text; the tests read it
// through pram_last_kernel()).  PRAM_NOTE_LAUNCH("family", a, b, c) goes immediately before every hipLaunchKernelGGL whose
// instantiation the problem size picks: a string literal and up to three template arguments (negative = none), a few word stores and
// no formatting — the text is made when somebody asks.  "family/variant" prints the variant as a last argument.
struct PramLaunchNote { const char* family; int a, b, c; };
extern thread_local PramLaunchNote g_pram_last_launch;
#define PRAM_NOTE_LAUNCH(family, a, b, c) (g_pram_last_launch = PramLaunchNote{family, (int)(a), (int)(b), (int)(c)})

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
