// Diagnostic build (r05): the layer3-shaped f16x3 BD forward (k_igemm_fwd_sk2) with in-kernel s_memtime
// stamps (fwd_sk_body PROF) - where a K-step of the loop spends its cycles.  Not part of the library:
//   hipcc --offload-arch=gfx950 -O3 -fPIC -shared -std=c++17 scripts/probe_sk.hip maxsquareloss_amd/csrc/bn.hip \
//         -o scripts/probe_sk.so
// driven by scripts/probe_sk.py.  The launch follows plan_fwd's BD f16x3 plan (dconv.hip), always with the image operand in registers.
#include "../maxsquareloss_amd/csrc/dconv.hip"

extern "C" int probe_bd_fwd(const float* x, const float* packed, float* y, int cin, int cout, int h, int w, int nimg,
                            int dil, const float* x_part, int x_npart, void* ws, size_t ws_bytes,
                            unsigned long long* prof, int with_prof, msl_stream_t stream) {
  hipStream_t st = as_stream(stream);
  const int P = nimg * h * w;
  const FwdPlan pl = plan_fwd(kMathH3P, 1, 9, cin, cout, P, 0, dil, nullptr);
  if (!pl.sk || pl.form.bm != 128 || pl.form.bform == kBLds) return MSL_ERR_SHAPE;
  FwdArgs a{};
  a.A = packed;
  a.B = x;
  a.C = y;
  a.M = cout;
  a.lda = pad_to(cout, kPackPad);
  a.H = h;
  a.W = w;
  a.P = P;
  a.cimg = cin;
  a.ncb = cdiv(cin, kCB);
  a.dil0 = dil;
  a.ksteps = pl.ksteps;
  a.kps = pl.kps;
  a.taps = 9;
  a.slab = (long long)cout * P;
  const long long f32 = (long long)pl.ksteps * kCB * a.lda;
  a.Ax6 = reinterpret_cast<const __bf16*>(packed + f32);
  a.bpart = x_part;
  a.bnpart = x_npart;
  a.ascale = packed + pack_tail_offset(f32) + kNPart;
  if (ws_bytes < fwd_piece_bytes(9, cout)) return MSL_ERR_WORKSPACE;
  SkArgs sk = pl.sched;
  sk.part = (float*)ws;
  const long long tiles = (long long)pl.tiles_m * pl.tiles_n, T = sk.T;
  const int nwk = kSkNW;
  sk.prof = prof;
  const dim3 grid(sk.tdp > 0 ? nwk : sk.NW), block(256);
  // with_prof: 1 stamps; 2, 4, 8, 6, 14 timing-only ablations, 16 a BN-apply of the image operand
  // (dconv_kernels.h fwd_sk_body PROF)
#define PROBE_CASE(V)                                                                                              \
  case V:                                                                                                          \
    hipLaunchKernelGGL((k_igemm_fwd_sk2<128, kSkBN, 1, 4, 1, 4, false, kMathH3P, false, true, false, V>), grid,     \
                       block, 0, st, a, sk);                                                                       \
    break;
  switch (with_prof) {
    PROBE_CASE(0)
    PROBE_CASE(1)
    PROBE_CASE(2)
    PROBE_CASE(4)
    PROBE_CASE(6)
    PROBE_CASE(8)
    PROBE_CASE(14)
    PROBE_CASE(16)

    default: return MSL_ERR_ARG;
  }
  MSL_CHECK_LAUNCH();
  if (T > 0)
    hipLaunchKernelGGL((k_sk_reduce<128, kSkBN>), dim3(128 * kSkBN / 1024, (unsigned)(tiles - sk.tdp)), block, 0, st,
                       a, sk);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

extern "C" int probe_workers(int cin, int cout, int h, int w, int nimg) {
  const int P = nimg * h * w;
  const SkArgs sk = plan_fwd(kMathH3P, 1, 9, cin, cout, P, 0, 1, nullptr).sched;
  return sk.tdp > 0 ? kSkNW : sk.NW;
}
