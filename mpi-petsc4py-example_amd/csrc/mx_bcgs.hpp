// mx_bcgs.hpp -- KSPBCGS (BiCGStab) on gfx950; part of mx_ksp.hip, which
// includes it after the CG and GMRES drivers (it uses their file-local
// helpers: dev_converged, Poller, SpmvTimer, Carve, ld2 / st2).
//
// van der Vorst's method in PETSc's arrangement, left preconditioning (B: the
// identity or Jacobi's dinv), preconditioned norm:
//
//   R = B (b - A x);  dp = ||R||;  converged(0, dp);  RP = R;  rho = RP . R
//   iteration i:
//     rho == 0 -> DIVERGED_BREAKDOWN
//     P = R + beta (P - omega V)     beta = (rho / rhoold) (alphaold / omegaold); i == 0: P = R
//     V = B A P;  d1 = V . RP        d1 == 0 -> DIVERGED_BREAKDOWN
//     S = R - alpha V                alpha = rho / d1
//     T = B A S;  d1 = S . T, d2 = T . T
//     d2 == 0: x += alpha P, its += 1, CONVERGED_RTOL when S . S == 0 else DIVERGED_BREAKDOWN
//     x += alpha P + omega S         omega = d1 / d2
//     R = S - omega T;  dp = ||R||;  its += 1;  converged(its, dp)
//
// Per iteration: two MatMults (Jacobi fused) and five vector passes --
//   bcgs_p     P = R + beta (P - omega V)                       reads R P V, writes P
//   bcgs_dot1  V . RP                                           reads V RP
//   bcgs_s     S = R - alpha V                                  reads R V, writes S
//   bcgs_dot2  S . T, T . T, S . S                              reads S T
//   bcgs_xr    x += alpha P + omega S; R = S - omega T;         reads x P S T RP, writes x R
//              ||R||^2 and RP . R (the next rho)
// 18 n doubles of vector traffic.  Every scalar lives in KspState::bc.  One
// rank: each reducing pass folds its partials in-launch and the workgroup that
// folded runs the scalar step.  P > 1: finish_reduce, one all-reduce of the
// grouped values (1, 3 and 2 doubles per iteration), then the step as a
// one-thread kernel.  Every pass is a no-op once the solve has stopped.
//
// Rows go in 16-byte pairs when every operand is 16-byte aligned (the same
// walk on scalars otherwise, so the partial sums do not depend on alignment);
// each thread has two pairs' loads in flight.  Operands not read again soon
// are loaded non-temporally (ldn); bcgs_dot2's S and T, which bcgs_xr reads
// next, and the stores (P and S feed the MatMults, R the next bcgs_p) are plain.

constexpr int BCGS_BLOCKS = 4096;   // grid cap of the vector passes (fixed: deterministic partials)

// what the host polls (Poller): at a stop, HW_DONE = 1 + the iterations begun
// (a breakdown inside iteration i counts it as begun); HW_PROGRESS = its after
// every iteration that did not stop the solve.  A stop with DONE - 1 <= t has
// PROGRESS < t, so "DONE != 0 or PROGRESS >= t" ends on DONE alone and every
// rank decides the same
__device__ __forceinline__ void bcgs_stop(KspState *s, int reason, int begun, int *hw) {
  stop(s, reason);
  host_store(hw + HW_DONE, begun + 1);
}

// after the initial pass: red[0] = ||R||^2 (= RP . R), red[1] = ||B b||^2 (nonzero guess)
__device__ void bcgs_init_step(KspState *s, double *hist, int *hw) {
  const double rr = s->red[0];
  const double dp = sqrt(rr), snorm = sqrt(s->red[1]);
  s->its = 0;
  s->bc.it = 0;
  s->bc.dp = dp;
  if (hist) hist[0] = dp;
  const int reason = dev_converged(s, 0, dp, s->guess_zero, snorm);
  if (reason) { bcgs_stop(s, reason, 0, hw); return; }
  s->bc.rho = rr;
  s->bc.omega = 1.0;
  if (rr == 0.0) bcgs_stop(s, R_DIVERGED_BREAKDOWN, 1, hw);
}

// after bcgs_dot1: red[0] = V . RP
__device__ void bcgs_dot1_step(KspState *s, int *hw) {
  const double d1 = s->red[0];
  s->bc.d1 = d1;
  if (d1 == 0.0) bcgs_stop(s, R_DIVERGED_BREAKDOWN, s->bc.it + 1, hw);
}

// after bcgs_dot2: red[0..3) = S . T, T . T, S . S
__device__ void bcgs_dot2_step(KspState *s) {
  const double d1 = s->red[0], d2 = s->red[1];
  s->bc.ss = s->red[2];
  if (d2 == 0.0) { s->bc.tzero = 1; return; }
  s->bc.omega = d1 / d2;
}

// after bcgs_xr: red[0] = ||R||^2, red[1] = RP . R (bc.omega is this
// iteration's, bc.rho still the one the pass used)
__device__ void bcgs_xr_step(KspState *s, double *hist, int *hw) {
  const int its = s->bc.it + 1;
  s->its = its;
  if (s->bc.tzero) {
    s->bc.dp = 0.0;
    if (hist) hist[its] = 0.0;
    bcgs_stop(s, s->bc.ss == 0.0 ? R_CONVERGED_RTOL : R_DIVERGED_BREAKDOWN, its, hw);
    return;
  }
  const double rho = s->bc.rho, alpha = rho / s->bc.d1, omega = s->bc.omega;
  const double dp = sqrt(s->red[0]), rhon = s->red[1];
  s->bc.dp = dp;
  if (hist) hist[its] = dp;
  int reason = dev_converged(s, its, dp, true, 0.0);
  if (!reason && its >= s->top.max_it) reason = R_DIVERGED_ITS;
  if (reason) { bcgs_stop(s, reason, its, hw); return; }
  if (rhon == 0.0) { bcgs_stop(s, R_DIVERGED_BREAKDOWN, its + 1, hw); return; }
  s->bc.beta = (rhon / rho) * (alpha / omega);
  s->bc.rho = rhon;
  s->bc.it = its;
  host_store(hw + HW_PROGRESS, its);
}

// P > 1: the step after the all-reduce, one thread
__global__ void bcgs_step_kernel(KspState *s, int which, double *hist, int *hw) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (which == 0) { bcgs_init_step(s, hist, hw); return; }
  if (s->top.done) return;
  if (which == 1) bcgs_dot1_step(s, hw);
  else if (which == 2) bcgs_dot2_step(s);
  else bcgs_xr_step(s, hist, hw);
}

// the result into the host's words; the solve's last kernel
__global__ void bcgs_tail_kernel(KspState *s, int *hw) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const long long t_end = wall_clock64();
  host_store(hw + HW_ITS, s->its);
  host_store(hw + HW_REASON, s->reason);
  const unsigned long long dp = __builtin_bit_cast(unsigned long long, s->bc.dp);
  __hip_atomic_store(reinterpret_cast<unsigned long long *>(hw + HW_DP), dp, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(reinterpret_cast<long long *>(hw + HW_TICKS), t_end - s->t_start, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
}

// R = RP = B (b - A x) (ax null: B b; x_out set: x = 0), partials of ||R||^2
// and, with ax, of ||B b||^2 (KSPConvergedDefault's rnorm0 under a nonzero guess)
__global__ void __launch_bounds__(256) bcgs_init_kernel(int64_t n, const double *__restrict__ b,
                                                        const double *__restrict__ ax, const Jac jac,
                                                        double *__restrict__ R, double *__restrict__ RP,
                                                        double *__restrict__ x_out, double *__restrict__ partials,
                                                        const Fold fold, KspState *__restrict__ s,
                                                        double *__restrict__ hist, int *__restrict__ hw) {
  double v[2] = {0.0, 0.0};
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const double bi = b[i];
    const double ri = papply(jac, ax ? fma(-1.0, ax[i], bi) : bi, i);
    R[i] = ri;
    RP[i] = ri;
    if (x_out) x_out[i] = 0.0;
    v[0] += ri * ri;
    if (ax) {
      const double zb = papply(jac, bi, i);
      v[1] += zb * zb;
    }
  }
  if (!fold.cnt) { block_sum_to_partials<2>(v, partials, gridDim.x); return; }
  if (block_fold<2>(v, partials, fold) && threadIdx.x == 0) bcgs_init_step(s, hist, hw);
}

// the pair walk: ld(k) loads pair k's operands, fn(k, operands) finishes it;
// one(i) is the odd last row (workgroup 0, thread 0, after its pairs)
template <class LD, class FN, class ONE>
__device__ __forceinline__ void bcgs_walk(int64_t n, LD ld, FN fn, ONE one) {
  const int64_t np = n >> 1, stride = (int64_t)gridDim.x * 256;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < np; k += 2 * stride) {
    const int64_t k2 = k + stride;
    const bool two = k2 < np;
    const auto a = ld(k);
    const auto c = ld(two ? k2 : k);
    fn(k, a);
    if (two) fn(k2, c);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) one(n - 1);
}

// pair load of an operand that no later pass reads before it is rewritten (or
// only after the whole iteration's traffic): non-temporal, so the memory-side
// cache keeps what the next MatMult and the next pass read instead (BCGS_NTL:
// 256^3 C4 solve 242.5 -> 211.4 ms, bcgs_xr 167 -> 147 us, bcgs_p 109 -> 81 us,
// the MatMult after them 70 -> 65 us; profiles/bcgs_nt_ab.txt)
#ifndef BCGS_NTL
#define BCGS_NTL 1
#endif
template <bool VEC> __device__ __forceinline__ dbl2 ldn(const double *__restrict__ v, int64_t k) {
  if constexpr (!BCGS_NTL) return ld2<VEC>(v, k);
  else if constexpr (VEC) return __builtin_nontemporal_load(reinterpret_cast<const dbl2 *>(v) + k);
  else return dbl2{__builtin_nontemporal_load(v + 2 * k), __builtin_nontemporal_load(v + 2 * k + 1)};
}
struct Bp2 { dbl2 a, b; };
struct Bp3 { dbl2 a, b, c; };
struct Bp5 { dbl2 a, b, c, d, e; };

// P = R + beta (P - omega V); iteration 0: P = R (P and V are not read: the
// work space may be uninitialised)
template <bool VEC>
__global__ void __launch_bounds__(256) bcgs_p_kernel(int64_t n, const KspState *__restrict__ s,
                                                     const double *__restrict__ R, const double *__restrict__ V,
                                                     double *__restrict__ P) {
  if (s->top.done) return;
  const double beta = s->bc.beta, omega = s->bc.omega;
  if (s->bc.it == 0) {
    bcgs_walk(n, [&](int64_t k) { return ldn<VEC>(R, k); }, [&](int64_t k, dbl2 r) { st2<VEC>(P, k, r); },
              [&](int64_t i) { P[i] = R[i]; });
    return;
  }
  auto row = [&](double r, double p, double v) { return r + beta * (p - omega * v); };
  bcgs_walk(n, [&](int64_t k) { return Bp3{ldn<VEC>(R, k), ldn<VEC>(P, k), ldn<VEC>(V, k)}; },
            [&](int64_t k, const Bp3 &t) { st2<VEC>(P, k, dbl2{row(t.a.x, t.b.x, t.c.x), row(t.a.y, t.b.y, t.c.y)}); },
            [&](int64_t i) { P[i] = row(R[i], P[i], V[i]); });
}

// partials of V . RP
template <bool VEC>
__global__ void __launch_bounds__(256) bcgs_dot1_kernel(int64_t n, KspState *__restrict__ s,
                                                        const double *__restrict__ V, const double *__restrict__ RP,
                                                        double *__restrict__ partials, const Fold fold,
                                                        int *__restrict__ hw) {
  if (s->top.done) return;
  double v[1] = {0.0};
  bcgs_walk(n, [&](int64_t k) { return Bp2{ld2<VEC>(V, k), ldn<VEC>(RP, k)}; },   // (bcgs_s reads V next)
            [&](int64_t, const Bp2 &t) { v[0] += t.a.x * t.b.x; v[0] += t.a.y * t.b.y; },
            [&](int64_t i) { v[0] += V[i] * RP[i]; });
  if (!fold.cnt) { block_sum_to_partials<1>(v, partials, gridDim.x); return; }
  if (block_fold<1>(v, partials, fold) && threadIdx.x == 0) bcgs_dot1_step(s, hw);
}

// S = R - alpha V
template <bool VEC>
__global__ void __launch_bounds__(256) bcgs_s_kernel(int64_t n, const KspState *__restrict__ s,
                                                     const double *__restrict__ R, const double *__restrict__ V,
                                                     double *__restrict__ S) {
  if (s->top.done) return;
  const double alpha = s->bc.rho / s->bc.d1;
  bcgs_walk(n, [&](int64_t k) { return Bp2{ldn<VEC>(R, k), ldn<VEC>(V, k)}; },
            [&](int64_t k, const Bp2 &t) { st2<VEC>(S, k, dbl2{t.a.x - alpha * t.b.x, t.a.y - alpha * t.b.y}); },
            [&](int64_t i) { S[i] = R[i] - alpha * V[i]; });
}

// partials of S . T, T . T, S . S
template <bool VEC>
__global__ void __launch_bounds__(256) bcgs_dot2_kernel(int64_t n, KspState *__restrict__ s,
                                                        const double *__restrict__ S, const double *__restrict__ T,
                                                        double *__restrict__ partials, const Fold fold) {
  if (s->top.done) return;
  double v[3] = {0.0, 0.0, 0.0};
  auto row = [&](double a, double t) { v[0] += a * t; v[1] += t * t; v[2] += a * a; };
  bcgs_walk(n, [&](int64_t k) { return Bp2{ld2<VEC>(S, k), ld2<VEC>(T, k)}; },
            [&](int64_t, const Bp2 &t) { row(t.a.x, t.b.x); row(t.a.y, t.b.y); },
            [&](int64_t i) { row(S[i], T[i]); });
  if (!fold.cnt) { block_sum_to_partials<3>(v, partials, gridDim.x); return; }
  if (block_fold<3>(v, partials, fold) && threadIdx.x == 0) bcgs_dot2_step(s);
}

// x += alpha P + omega S; R = S - omega T; partials of ||R||^2 and RP . R.
// T vanished (bc.tzero): x += alpha P only, the partials are zeros
template <bool VEC>
__global__ void __launch_bounds__(256) bcgs_xr_kernel(int64_t n, KspState *__restrict__ s,
                                                      const double *__restrict__ P, const double *__restrict__ S,
                                                      const double *__restrict__ T, const double *__restrict__ RP,
                                                      double *__restrict__ x, double *__restrict__ R,
                                                      double *__restrict__ partials, const Fold fold,
                                                      double *__restrict__ hist, int *__restrict__ hw) {
  if (s->top.done) return;
  const double alpha = s->bc.rho / s->bc.d1, omega = s->bc.omega;
  double v[2] = {0.0, 0.0};
  if (s->bc.tzero) {
    bcgs_walk(n, [&](int64_t k) { return Bp2{ld2<VEC>(x, k), ld2<VEC>(P, k)}; },
              [&](int64_t k, const Bp2 &t) { st2<VEC>(x, k, dbl2{t.a.x + alpha * t.b.x, t.a.y + alpha * t.b.y}); },
              [&](int64_t i) { x[i] = x[i] + alpha * P[i]; });
  } else {
    auto rnew = [&](double sv, double tv, double rp) {
      const double r = sv - omega * tv;
      v[0] += r * r; v[1] += rp * r;
      return r;
    };
    auto xnew = [&](double xv, double pv, double sv) { return xv + (alpha * pv + omega * sv); };
    bcgs_walk(n,
              [&](int64_t k) { return Bp5{ldn<VEC>(x, k), ldn<VEC>(P, k), ldn<VEC>(S, k), ldn<VEC>(T, k), ldn<VEC>(RP, k)}; },
              [&](int64_t k, const Bp5 &t) {
                st2<VEC>(x, k, dbl2{xnew(t.a.x, t.b.x, t.c.x), xnew(t.a.y, t.b.y, t.c.y)});
                const double r0 = rnew(t.c.x, t.d.x, t.e.x);
                const double r1 = rnew(t.c.y, t.d.y, t.e.y);
                st2<VEC>(R, k, dbl2{r0, r1});
              },
              [&](int64_t i) {
                x[i] = xnew(x[i], P[i], S[i]);
                R[i] = rnew(S[i], T[i], RP[i]);
              });
  }
  if (!fold.cnt) { block_sum_to_partials<2>(v, partials, gridDim.x); return; }
  if (block_fold<2>(v, partials, fold) && threadIdx.x == 0) bcgs_xr_step(s, hist, hw);
}

static void bcgs_solve(Mat *A, const mx_ksp_params &p, const Jac dinv, const double *b, double *x,
                       mx_ksp_result &res, double *hist_host) {
  Comm *c = A->comm;
  hipStream_t st = c->stream;
  const int64_t n = A->m;
  if (p.norm_type != MX_NORM_DEFAULT && p.norm_type != MX_NORM_PRECONDITIONED && p.norm_type != MX_NORM_NONE)
    fail(MX_ERR_UNSUPPORTED, "BiCGStab with left preconditioning supports the preconditioned norm only");
  const int normtype = p.norm_type == MX_NORM_NONE ? MX_NORM_NONE : MX_NORM_PRECONDITIONED;
  const bool fused = c->size == 1 && !g_knobs.force_coll;
  const size_t nv = (size_t)std::max<int64_t>(n, 1);
  const size_t npart = 3 * (size_t)BCGS_BLOCKS + 64;
  const size_t nhist = hist_host ? (size_t)p.max_it + 2 : 1;
  const size_t nax = p.guess_nonzero ? nv : 0;
  Carve cv(workspace(A, carve_size({nv, nv, nv, nv, nv, nv, nax, npart, nhist, 32})));
  double *R = cv.take(nv), *RP = cv.take(nv), *P = cv.take(nv), *V = cv.take(nv), *S = cv.take(nv), *T = cv.take(nv);
  double *ax = cv.take(nax), *part = cv.take(npart), *hist = cv.take(nhist), *one = cv.take(32);
  if (hist_host) HIPCHECK(hipMemsetAsync(hist, 0, sizeof(double) * nhist, st));   // as in CG
  double *hist_d = hist_host ? hist : nullptr;
  KspState *s = state_buf(A);
  const KspInit kin{p.rtol, p.atol, p.dtol, p.haptol, p.breakdowntol, p.max_it, normtype, !p.guess_nonzero, p.restart};
  ksp_state_init_kernel<<<1, 256, 0, st>>>(s, kin);
  HIPCHECK(hipGetLastError());
  vec_set(st, 1, 1.0, one);   // the MatMult's operand scale (SPMV_*_S: 1.0 * x is x)
  const int ntime = std::min(p.max_it, 4096);
  SpmvTimer timer((p.profile & 1) != 0, st, 2 * ntime);   // both MatMults
  SpmvTimer utimer((p.profile & 2) != 0, st, ntime);      // bcgs_xr
  SpmvTimer ptimer((p.profile & 4) != 0, st, ntime);      // bcgs_p
  timer.ext = utimer.ext = ptimer.ext = c->size == 1;

  Poller poller(A, st);
  int *hw = poller.hw;
  int *done = &s->top.done;
  // two pairs (four rows) per thread up to BCGS_BLOCKS workgroups, a grid-stride walk beyond
  const int g = (int)grid_for(cdiv(n, 4), 256, BCGS_BLOCKS);
  Fold fold;                 // one rank: every reducing pass folds into s->red
  if (fused) { fold.cnt = s->fold_upd; fold.out = s->red; fold.ntotal = fold.ncount = g; }
  // P > 1: the grouped values of a pass, one all-reduce, then its scalar step
  auto reduce = [&](int nvals, int which) {
    if (fused) return;
    finish_reduce(part, g, nvals, s->red, st, which ? done : nullptr);
    c->allreduce_sum(s->red, nvals);
    bcgs_step_kernel<<<1, 64, 0, st>>>(s, which, hist_d, hw);
    HIPCHECK(hipGetLastError());
  };

  if (p.guess_nonzero) mat_mult(A, x, ax);
  bcgs_init_kernel<<<g, 256, 0, st>>>(n, b, p.guess_nonzero ? ax : nullptr, dinv, R, RP,
                                      p.guess_nonzero ? nullptr : x, part, fold, s, hist_d, hw);
  HIPCHECK(hipGetLastError());
  reduce(2, 0);

  const int mm = dinv.mode ? SPMV_JACOBI_S : SPMV_PLAIN_S;
  const bool vec = aligned16({R, RP, P, V, S, T}), vecx = vec && aligned16({x});
#define BCGS_K(K, V16, ...) do { if (V16) K<true><<<g, 256, 0, st>>>(__VA_ARGS__); \
                                 else K<false><<<g, 256, 0, st>>>(__VA_ARGS__); } while (0)
#define BCGS_KT(K, V16, ...) do { if (V16) launch_timed(&K<true>, g, st, __VA_ARGS__); \
                                  else launch_timed(&K<false>, g, st, __VA_ARGS__); } while (0)
  auto iteration = [&]() {
    ptimer.begin();
    BCGS_KT(bcgs_p_kernel, vec, n, (const KspState *)s, (const double *)R, (const double *)V, P);
    ptimer.end();
    timer.begin();
    matmult_overlap(A, P, V, mm, dinv, nullptr, done, nullptr, nullptr, one);
    timer.end();
    BCGS_K(bcgs_dot1_kernel, vec, n, s, V, RP, part, fold, hw);
    reduce(1, 1);
    BCGS_K(bcgs_s_kernel, vec, n, s, R, V, S);
    timer.begin();
    matmult_overlap(A, S, T, mm, dinv, nullptr, done, nullptr, nullptr, one);
    timer.end();
    BCGS_K(bcgs_dot2_kernel, vec, n, s, S, T, part, fold);
    reduce(3, 2);
    utimer.begin();
    BCGS_KT(bcgs_xr_kernel, vecx, n, s, (const double *)P, (const double *)S, (const double *)T, (const double *)RP,
            x, R, part, fold, hist_d, hw);
    utimer.end();
    reduce(2, 3);
    HIPCHECK(hipGetLastError());
  };
#undef BCGS_K
#undef BCGS_KT

  // batches of `poll` iterations, polled one batch behind (Poller); the host
  // stops on a stop that lies within the batch it waited for, which every
  // rank sees alike (bcgs_stop); one rank stops on any
  const int poll = p.poll_every > 0 ? p.poll_every : 16;
  int i = 0, prev_end = 0, batches = 0;
  while (i < p.max_it) {
    for (int k = 0; k < poll && i < p.max_it; ++k, ++i) iteration();
    const int target = prev_end;
    prev_end = i;
    if (++batches < 2) continue;
    c->wait_until([&] { return poller.word(HW_DONE) != 0 || poller.word(HW_PROGRESS) >= target; }, st,
                  [&] { return (long long)poller.word(HW_PROGRESS); }, 0);
    const int dw = poller.word(HW_DONE);
    if (dw != 0 && (fused || dw - 1 <= target)) break;
  }
  bcgs_tail_kernel<<<1, 64, 0, st>>>(s, hw);
  HIPCHECK(hipGetLastError());
  c->wait_stream(st);
  res.its = poller.word(HW_ITS);
  res.reason = poller.word(HW_REASON);
  std::memcpy(&res.rnorm, (const void *)(hw + HW_DP), sizeof(double));
  long long ticks = 0;
  std::memcpy(&ticks, (const void *)(hw + HW_TICKS), sizeof(ticks));
  res.solve_ms = (double)ticks / wall_clock_khz(c->device);
  res.launched_its = i;
  timer.collect(res.spmv_ms, res.spmv_count);
  utimer.collect(res.upd_ms, res.upd_count);
  ptimer.collect(res.pb_ms, res.pb_count);
  if (hist_host)
    HIPCHECK(hipMemcpy(hist_host, hist, sizeof(double) * ((size_t)res.its + 1), hipMemcpyDeviceToHost));
}
