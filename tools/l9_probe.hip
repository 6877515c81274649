// Probe of the nine-limb lazy field arithmetic (halo2_vectordb_amd/csrc/limb9.hpp on the product cores of field.hpp, and the MSM
// accumulator of ec_l9.hpp), primitive by primitive, for tests/test_l9_cpu.py and tests/test_gpu_l9.py, which hold every output to
// Python integers:  hipcc -O2 -std=c++17 --offload-arch=gfx950 -o l9_probe tools/l9_probe.hip
//   l9_probe --host   cases.bin out.bin    the C++ forms (the #else branches of field.hpp); calls no HIP runtime function
//   l9_probe --device cases.bin out.bin    one plain kernel per op, one thread per case: the inline-asm forms of field.hpp are what runs
// Both files are little-endian uint32 words: MAGIC, number of blocks, then per block  op, field (0 = Fr, 1 = Fq), count  followed by
// count records of NIN[op] words (cases) resp. NOUT[op] words (results).  Limb arrays are 9 raw words, u256 values 8 words.
//   op  name              in                                            out
//    0  mont_core29       A B                                           9 limbs
//    1  mont_core29_2     A1 B1 A2 B2                                   9
//    2  mont_sqr_core29   A                                             9
//    3  shoup_core29      V W WQ                                        9
//    4  from_mont         a (u256)                                      u256
//    5  mont_mul          a b (u256)                                    u256
//    6  l9_split          a (u256)                                      9
//    7  l9_split32        a (u256)                                      9
//    8  l9_pack           L                                             u256
//    9  l9_renorm         L                                             9
//   10  l9_carry          L                                             9
//   11  l9_add            A B                                           9
//   12  l9_sub            A T CKP                                       9
//   13  l9_neg            T CKP                                         9
//   14  l9_canon          L                                             u256
//   15  l9_is_zero_mod    L                                             1 word
//   16  l9_canon_wide     L                     (Fr, device only)       u256
//   17  l9_offset_limbs   K                     (host only)             9 limbs, cmax (a double: 2 words)
//   18  shoup_pair29      w (u256)              (Fr, host only)         18
//   19  madd_l9           x y zz zzz ident, px py (u256), neg  (Fq, device only)   x y zz zzz ident
//   20  mdbl_l9           x y                   (Fq, device only)       x y zz zzz ident
//   21  gate step x n     h, y32 a b c d sel (u256), C2, n              h after n steps of k_gate_eval's loop body (polyops.hip), l9_canon of it
//   22  madd_l9 chain     x y zz zzz ident, 64 x (px py neg)   (Fq, device only)   64 x (x y zz zzz ident): the accumulator after every step
// l9_canon_wide, madd_l9 and mdbl_l9 are device functions (they are the kernels' own text), so only --device reaches them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../halo2_vectordb_amd/csrc/ec_l9.hpp"
#include "../halo2_vectordb_amd/csrc/limb9.hpp"
using namespace vdb;

#define L9P_MAGIC 0x4c395042u
#define L9P_NOPS 23
#define L9P_CHAIN 64
static constexpr uint32_t NIN[L9P_NOPS] = {18, 36, 9, 27, 8, 16, 8, 8, 9, 9, 9, 18, 27, 18, 9, 9, 9, 1, 8, 54, 18, 67, 37 + L9P_CHAIN * 17};
static constexpr uint32_t NOUT[L9P_NOPS] = {9, 9, 9, 9, 8, 8, 9, 9, 8, 9, 9, 9, 9, 9, 8, 1, 8, 11, 18, 37, 37, 17, L9P_CHAIN * 37};
// 0: host and device; 1: device only; 2: host only
static constexpr int WHERE[L9P_NOPS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 2, 1, 1, 0, 1};

HD L9 get9(const uint32_t* p) {
  L9 r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.l[k] = p[k];
  return r;
}
HD void put9(uint32_t* p, const L9& v) {
#pragma unroll
  for (int k = 0; k < 9; k++) p[k] = v.l[k];
}
HD u256 get8(const uint32_t* p) {
  u256 r;
#pragma unroll
  for (int k = 0; k < 8; k++) r.w[k] = p[k];
  return r;
}
HD void put8(uint32_t* p, const u256& v) {
#pragma unroll
  for (int k = 0; k < 8; k++) p[k] = v.w[k];
}

// the ops that exist on both sides
template <class M, int OP>
HD void eval_hd(const uint32_t* in, uint32_t* out) {
  if constexpr (OP == 0) {
    uint32_t A[9], B[9], o[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
      A[k] = in[k];
      B[k] = in[9 + k];
    }
    mont_core29<M>(o, A, B);
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = o[k];
  } else if constexpr (OP == 1) {
    uint32_t A1[9], B1[9], A2[9], B2[9], o[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
      A1[k] = in[k];
      B1[k] = in[9 + k];
      A2[k] = in[18 + k];
      B2[k] = in[27 + k];
    }
    mont_core29_2<M>(o, A1, B1, A2, B2);
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = o[k];
  } else if constexpr (OP == 2) {
    uint32_t A[9], o[9];
#pragma unroll
    for (int k = 0; k < 9; k++) A[k] = in[k];
    mont_sqr_core29<M>(o, A);
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = o[k];
  } else if constexpr (OP == 3) {
    uint32_t V[9], W[9], WQ[9], o[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
      V[k] = in[k];
      W[k] = in[9 + k];
      WQ[k] = in[18 + k];
    }
    shoup_core29<M>(o, V, W, WQ);
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = o[k];
  } else if constexpr (OP == 4) {
    put8(out, from_mont<M>(get8(in)));
  } else if constexpr (OP == 5) {
    put8(out, mont_mul<M>(get8(in), get8(in + 8)));
  } else if constexpr (OP == 6) {
    put9(out, l9_split(get8(in)));
  } else if constexpr (OP == 7) {
    put9(out, l9_split32(get8(in)));
  } else if constexpr (OP == 8) {
    put8(out, l9_pack(get9(in)));
  } else if constexpr (OP == 9) {
    L9 x = get9(in);
    l9_renorm(x);
    put9(out, x);
  } else if constexpr (OP == 10) {
    L9 x = get9(in);
    l9_carry(x);
    put9(out, x);
  } else if constexpr (OP == 11) {
    put9(out, l9_add(get9(in), get9(in + 9)));
  } else if constexpr (OP == 12) {
    uint32_t ckp[9];
#pragma unroll
    for (int k = 0; k < 9; k++) ckp[k] = in[18 + k];
    put9(out, l9_sub(get9(in), get9(in + 9), ckp));
  } else if constexpr (OP == 13) {
    uint32_t ckp[9];
#pragma unroll
    for (int k = 0; k < 9; k++) ckp[k] = in[9 + k];
    put9(out, l9_neg(get9(in), ckp));
  } else if constexpr (OP == 14) {
    put8(out, l9_canon<M>(get9(in)));
  } else if constexpr (OP == 15) {
    out[0] = l9_is_zero_mod<M>(get9(in)) ? 1u : 0u;
  } else if constexpr (OP == 21) {
    // the loop body of k_gate_eval (polyops.hip), composed from the same primitives, fed back n times
    L9 h = get9(in);
    const L9 Y = l9_split(get8(in + 9));
    const u256 a = get8(in + 17), b = get8(in + 25), c = get8(in + 33), d = get8(in + 41), sel = get8(in + 49);
    uint32_t c2[9];
#pragma unroll
    for (int k = 0; k < 9; k++) c2[k] = in[57 + k];
    const uint32_t n = in[66];
    for (uint32_t it = 0; it < n; it++) {
      const L9 q32 = l9_split32(sel);
      const L9 bc = l9_mul<M>(l9_split(b), l9_split32(c));
      const L9 g = l9_sub(l9_add(l9_split(a), bc), l9_split(d), c2);
      h = l9_mul2<M>(h, Y, g, q32);
    }
    put9(out, h);
    put8(out + 9, l9_canon<M>(h));
  }
}

__device__ __forceinline__ void put_acc(uint32_t* out, const AccL9& acc, bool ident) {
  put9(out, acc.x);
  put9(out + 9, acc.y);
  put9(out + 18, acc.zz);
  put9(out + 27, acc.zzz);
  out[36] = ident ? 1u : 0u;
}
__device__ __forceinline__ void get_acc(const uint32_t* in, AccL9& acc, bool& ident) {
  acc.x = get9(in);
  acc.y = get9(in + 9);
  acc.zz = get9(in + 18);
  acc.zzz = get9(in + 27);
  ident = in[36] != 0;
}
// the device functions of the kernels
template <class M, int OP>
__device__ __forceinline__ void eval_dev(const uint32_t* in, uint32_t* out, const MsmL9Consts& K) {
  if constexpr (OP == 16) {
    put8(out, l9_canon_wide(get9(in)));
  } else if constexpr (OP == 19) {
    AccL9 acc;
    bool ident;
    get_acc(in, acc, ident);
    Affine p;
    p.x = get8(in + 37);
    p.y = get8(in + 45);
    madd_l9(acc, ident, p, in[53] != 0, K);
    put_acc(out, acc, ident);
  } else if constexpr (OP == 20) {
    AccL9 acc;
    acc.x = acc.y = acc.zz = acc.zzz = get9(in);   // (overwritten, or unspecified when the result is the identity)
    bool ident = false;
    mdbl_l9(acc, ident, get9(in), get9(in + 9), K);
    put_acc(out, acc, ident);
  } else if constexpr (OP == 22) {
    AccL9 acc;
    bool ident;
    get_acc(in, acc, ident);
    for (int s = 0; s < L9P_CHAIN; s++) {
      const uint32_t* q = in + 37 + 17 * s;
      Affine p;
      p.x = get8(q);
      p.y = get8(q + 8);
      madd_l9(acc, ident, p, q[16] != 0, K);
      put_acc(out + 37 * s, acc, ident);
    }
  } else {
    eval_hd<M, OP>(in, out);
  }
}

template <class M, int OP>
__global__ __launch_bounds__(64) void k_eval(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, MsmL9Consts K) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  eval_dev<M, OP>(in + (size_t)t * NIN[OP], out + (size_t)t * NOUT[OP], K);
}

static int hip_bad(hipError_t e, const char* what) {
  if (e == hipSuccess) return 0;
  fprintf(stderr, "l9_probe: %s: %s\n", what, hipGetErrorString(e));
  return 1;
}
template <class M, int OP>
static int run_device(const uint32_t* in, uint32_t* out, uint32_t n, const MsmL9Consts& K) {
  uint32_t *din = nullptr, *dout = nullptr;
  const size_t bi = (size_t)n * NIN[OP] * 4, bo = (size_t)n * NOUT[OP] * 4;
  int bad = hip_bad(hipMalloc(&din, bi), "hipMalloc") || hip_bad(hipMalloc(&dout, bo), "hipMalloc");
  bad = bad || hip_bad(hipMemcpy(din, in, bi, hipMemcpyHostToDevice), "hipMemcpy (in)");
  if (!bad) {
    hipLaunchKernelGGL((k_eval<M, OP>), dim3((n + 63) / 64), dim3(64), 0, 0, din, dout, n, K);
    bad = hip_bad(hipGetLastError(), "launch") || hip_bad(hipDeviceSynchronize(), "kernel");
  }
  bad = bad || hip_bad(hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost), "hipMemcpy (out)");
  if (din) bad = hip_bad(hipFree(din), "hipFree") || bad;
  if (dout) bad = hip_bad(hipFree(dout), "hipFree") || bad;
  return bad;
}
template <class M, int OP>
static int run_host(const uint32_t* in, uint32_t* out, uint32_t n) {
  for (uint32_t t = 0; t < n; t++) {
    const uint32_t* i = in + (size_t)t * NIN[OP];
    uint32_t* o = out + (size_t)t * NOUT[OP];
    if constexpr (OP == 17) {
      const double cmax = l9_offset_limbs<M>(i[0], o);
      memcpy(o + 9, &cmax, 8);
    } else if constexpr (OP == 18) {
      shoup_pair29(get8(i), o);
    } else {
      eval_hd<M, OP>(i, o);
    }
  }
  return 0;
}
template <int OP>
static int run_op(int op, bool device, uint32_t mod, const uint32_t* in, uint32_t* out, uint32_t n, const MsmL9Consts& K) {
  if constexpr (OP < L9P_NOPS) {
    if (op != OP) return run_op<OP + 1>(op, device, mod, in, out, n, K);
    if ((WHERE[OP] == 1 && !device) || (WHERE[OP] == 2 && device)) {
      fprintf(stderr, "l9_probe: op %d does not exist in this mode\n", op);
      return 1;
    }
    if ((OP == 16 || OP == 18) && mod != 0) {
      fprintf(stderr, "l9_probe: op %d is over Fr\n", op);
      return 1;
    }
    if ((OP == 19 || OP == 20 || OP == 22) && mod != 1) {
      fprintf(stderr, "l9_probe: op %d is over Fq\n", op);
      return 1;
    }
    if constexpr (WHERE[OP] == 2) {
      return mod ? run_host<FqParams, OP>(in, out, n) : run_host<FrParams, OP>(in, out, n);
    } else if constexpr (WHERE[OP] == 1) {
      return mod ? run_device<FqParams, OP>(in, out, n, K) : run_device<FrParams, OP>(in, out, n, K);
    } else {
      if (device) return mod ? run_device<FqParams, OP>(in, out, n, K) : run_device<FrParams, OP>(in, out, n, K);
      return mod ? run_host<FqParams, OP>(in, out, n) : run_host<FrParams, OP>(in, out, n);
    }
  } else {
    fprintf(stderr, "l9_probe: unknown op %d\n", op);
    return 1;
  }
}

int main(int argc, char** argv) {
  if (argc != 4 || (strcmp(argv[1], "--host") && strcmp(argv[1], "--device"))) {
    fprintf(stderr, "usage: l9_probe --host|--device cases.bin out.bin\n");
    return 2;
  }
  const bool device = !strcmp(argv[1], "--device");
  FILE* f = fopen(argv[2], "rb");
  if (!f) {
    fprintf(stderr, "l9_probe: cannot read %s\n", argv[2]);
    return 2;
  }
  std::vector<uint32_t> in;
  {
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
  }
  if (in.size() < 2 || in[0] != L9P_MAGIC) {
    fprintf(stderr, "l9_probe: not a case file\n");
    return 2;
  }
  // the MSM's constants, as vdb_msm builds them (msm.hip)
  MsmL9Consts K;
  l9_offset_limbs<FqParams>(2, K.c2);
  l9_offset_limbs<FqParams>(8, K.c8);
  K.one_rp = to_mont<Fq>(u256_from_u64(32));
  K.to_std = mont_one<Fq>();
  K.to_rp = to_mont<Fq>(u256_from_u64(1024));
  std::vector<uint32_t> out = {L9P_MAGIC, in[1]};
  size_t pos = 2;
  for (uint32_t b = 0; b < in[1]; b++) {
    if (pos + 3 > in.size()) {
      fprintf(stderr, "l9_probe: truncated case file (block %u)\n", b);
      return 2;
    }
    const uint32_t op = in[pos], mod = in[pos + 1], n = in[pos + 2];
    pos += 3;
    if (op >= L9P_NOPS || mod > 1 || n == 0 || (in.size() - pos) / NIN[op] < n) {
      fprintf(stderr, "l9_probe: bad block %u (op %u, field %u, %u cases)\n", b, op, mod, n);
      return 2;
    }
    out.push_back(op);
    out.push_back(mod);
    out.push_back(n);
    const size_t o0 = out.size();
    out.resize(o0 + (size_t)n * NOUT[op]);
    if (run_op<0>((int)op, device, mod, in.data() + pos, out.data() + o0, n, K)) return 1;
    pos += (size_t)n * NIN[op];
  }
  if (pos != in.size()) {
    fprintf(stderr, "l9_probe: %zu words after the last block\n", in.size() - pos);
    return 2;
  }
  f = fopen(argv[3], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f)) {
    fprintf(stderr, "l9_probe: cannot write %s\n", argv[3]);
    return 2;
  }
  return 0;
}
