// hashmix.h -- the counter-based 32-bit hash shared by meshclean.hip (RANSAC draws), depthcloud.hip
// (pixel sampling keys, section 19) and mcmc.hip (noise and sampling draws, section 36): two rounds of a 32-bit finaliser over
// (seed, i, draw).  The restatements under tests/ hold the same arithmetic in uint32.
#pragma once
#include <stdint.h>

namespace {

__device__ __forceinline__ uint32_t mix32(uint32_t seed, uint32_t i, uint32_t draw) {
    uint32_t x = seed * 0x9E3779B1u + i * 0x85EBCA77u + draw * 0xC2B2AE3Du + 0x27D4EB2Fu;
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    x += i;
    x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12; x *= 0x297A2D39u; x ^= x >> 15;
    return x;
}

}  // namespace
