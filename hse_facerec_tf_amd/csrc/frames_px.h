// The per-pixel and per-tile device bodies of the frame kernels: a pixel as a dword, four pixels as one 12-byte unit, the byte forms.
// frames.hip (libhsefr_frames.so: a same-size stack, a frame is a grid index) and mixed_frames.hip (libhsefr_mixed.so: a packed buffer,
// a frame's place and size come from a table) compile this same code, so a frame's bytes are the same whichever entry moved them.
//
// The byte permutes are shifts and masks of 24-bit values, nothing that saturates: hipcc has no reason to select v_ashr_pk_u8_i32 here
// (tools/isa_lint.py refuses it, DESIGN.md lesson 36), and the 12-byte stores carry the gfx950 store-data guard (lesson 14).
#pragma once
#include <hip/hip_runtime.h>

namespace hsefr {

namespace {

// 12 bytes = 4 pixels, 4-byte aligned: one global_load_dwordx3 / global_store_dwordx3
struct __attribute__((aligned(4))) Px4 {
    unsigned a, b, c;
};

// a pixel as a dword: channel 0 in bits 0..7, channel 1 in 8..15, channel 2 in 16..23, bits 24..31 zero
__device__ __forceinline__ unsigned swap_02(unsigned p) { return ((p & 0xffu) << 16) | (p & 0xff00u) | ((p >> 16) & 0xffu); }

__device__ __forceinline__ void unpack4(const Px4& v, bool swap, unsigned p[4]) {
    p[0] = v.a & 0xffffffu;
    p[1] = ((v.a >> 24) | (v.b << 8)) & 0xffffffu;
    p[2] = ((v.b >> 16) | (v.c << 16)) & 0xffffffu;
    p[3] = v.c >> 8;
    if (swap) {
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = swap_02(p[k]);
    }
}

__device__ __forceinline__ Px4 pack4(unsigned p0, unsigned p1, unsigned p2, unsigned p3) {
    Px4 v;
    v.a = p0 | (p1 << 24);
    v.b = (p1 >> 8) | (p2 << 16);
    v.c = (p2 >> 16) | (p3 << 8);
    return v;
}

__device__ __forceinline__ void store_px4(unsigned char* at, const Px4& v) {
    *reinterpret_cast<Px4*>(at) = v;
    asm volatile("s_nop 1" ::: "memory");      // gfx950 store-data hazard: two wait states behind a wide store (tools/isa_lint.py)
}

__device__ __forceinline__ unsigned load_pixel(const unsigned char* at, bool swap) {
    const unsigned c0 = at[0], c1 = at[1], c2 = at[2];
    return swap ? (c2 | (c1 << 8) | (c0 << 16)) : (c0 | (c1 << 8) | (c2 << 16));
}

__device__ __forceinline__ void store_pixel(unsigned char* at, unsigned p) {
    at[0] = (unsigned char)(p & 0xffu);
    at[1] = (unsigned char)((p >> 8) & 0xffu);
    at[2] = (unsigned char)((p >> 16) & 0xffu);
}

}  // namespace

}  // namespace hsefr
