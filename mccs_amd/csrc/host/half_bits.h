// half_bits.h — binary16 / bfloat16 bit patterns on the host: conversion to and
// from binary32, round to nearest even (what v_cvt_f16_f32 / v_cvt_pk_bf16_f32
// do on the device).  Shared by the host-thread ring (host_ring.cpp) and the
// op-argument encoders (api.cpp mccsRedOpArgFromDouble / mccsAvgOp).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace mccs {

inline float h2f(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1f, man = h & 0x3ffu;
  uint32_t u;
  if (exp == 0) {
    float v = std::ldexp((float)man, -24);
    return sign ? -v : v;
  }
  if (exp == 31) u = sign | 0x7f800000u | (man << 13);
  else u = sign | ((exp + 112) << 23) | (man << 13);
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

inline uint16_t f2h(float f) {  // round to nearest even
  uint32_t u;
  std::memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
  if (a >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (a > 0x7f800000u ? 0x200u : 0));
  if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);
  if (a < 0x38800000u) {
    float v;
    std::memcpy(&v, &a, 4);
    return (uint16_t)(sign | (uint32_t)std::nearbyint(v * 16777216.0f));
  }
  uint32_t h = (((a >> 23) - 112) << 10) | ((a & 0x7fffffu) >> 13);
  const uint32_t rem = a & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h += 1;
  return (uint16_t)(sign | h);
}

inline float b2f(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

inline uint16_t f2b(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

}  // namespace mccs
