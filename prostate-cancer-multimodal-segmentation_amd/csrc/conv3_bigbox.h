// What the two big-box 3x3x3 convolution kernels share (conv3_big.hip: 32x32x16 MFMAs,
// conv3_b16.hip: 16x16x32), and the pack16 layout that conv3_pack.hip writes for the latter; gfx950.
#pragma once
#include "common.h"

namespace {

// the 8 x 8 x 16 box of conv3_fwd_big_kernel (conv3_big.hip); the 8-deep boxes and the halo
// planes of conv3_fwd_b16_kernel are the same (B6G / B6W, conv3_b16.hip)
constexpr int kBgThreads = 512;  // 8 waves = 4 M-groups x 2 N-tiles, two waves per SIMD
constexpr int kBgHH = 10, kBgHW = 18;
constexpr int kBgBD = 8;                                                  // box depth
constexpr int kBgMT = 8;                                                  // M-tiles per wave
constexpr int kBgHalo = (kBgBD + 2) * kBgHH * kBgHW;                      // rows x 32 B
constexpr int kBgPieces = (2 * kBgHalo + kBgThreads - 1) / kBgThreads;    // DMA pieces / thread (8)
// pieces pc = tid + 512 j; the last round (j = 7) holds real rows only for wave 0: the other
// waves aim it at a 1 KiB dummy slot (out-of-range source: no memory traffic) so every wave
// issues the same count; a buffer holds rows up to wave 0's last piece
constexpr int kBgBuf = ((kBgPieces - 1) * kBgThreads + 64) * 16;
constexpr int kBgDummy = 1024;
// ablation builds only (tests/tools/big_abl.py; 0 in the product): 1 halo DMA reads nothing
// (out-of-range source, the same instructions), 2 no output stores, 4 no MFMAs (operands still
// read), 8 no weight loads after the prologue, 16 no A-fragment LDS reads
#ifndef BG_ABL
#define BG_ABL 0
#endif

// hidden 16-B global load (the compiler's waitcnt pass does not count it): retired by
// vm_wait2<N>, which also orders the register's readers after the wait
__device__ __forceinline__ void gload16(s16x8_t& dst, const void* ptr) {
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(ptr) : "memory");
}
// the same through a buffer descriptor (bounds-checked: out of range reads zeros), one VGPR
// byte offset per address, immediate offset Imm
template <int Imm> __device__ __forceinline__ void bload16(s16x8_t& dst, i32x4_t rsrc, uint32_t voff) {
  asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen offset:%3" : "=v"(dst) : "v"(voff), "s"(rsrc), "n"(Imm)
               : "memory");
}
template <int N> __device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// conv3_fwd_b16_kernel walks a 16-channel chunk as pairs of taps (K = 32)
constexpr int kB6Steps = 14;                       // tap pairs per chunk
// pack16 layout (conv3_fwd_b16_kernel's B operand): element (16-chunk c, tap pair s, row j,
// lane group g, element e) = w[j][16 c + 8 (g & 1) + e][tap 2 s + (g >> 1)] (tap 27: zero), in
// 1 KiB blocks (c, s, j / 16) of lanes l = 16 g + j % 16 -- the v_mfma_f32_16x16x32_bf16 B
// fragment of that (tap pair, 16-row tile).  J % 16 == 0, Kdim % 16 == 0.
__host__ __device__ inline long pack16_off(int c, int s, int j, int g, int J) {
  return (((long)c * kB6Steps + s) * (J >> 4) + (j >> 4)) * 512 + (g * 16 + (j & 15)) * 8;
}

}  // namespace
