// Batched pose-graph optimiser (include/sship.h "Pose graph"): the objective of GlobalPoseGraph::optimize_and_get_all
// (BetweenFactor<Pose3> on the odometry chain and the loop closures, Huber on the loops, node 0 fixed) under the pose-only solver's
// Levenberg-Marquardt schedule, with the reference's drop-the-last-loop retry inside the launch.
//   k_pg_solve   one 256-thread workgroup per graph; the grid is min(graphs, kPgResident) workgroups that walk the graphs, each with a
//                workspace slice of its own, so a graph sees nothing of the others.
//     setup      presence of every odometry slot and loop record;  per attempt: the separators (loop endpoints) and the segment starts
//                in ascending node index (one wave, ballot compaction).
//     linearise  one thread per edge: r~, w and the two whitened 6x6 blocks (workspace);  then one thread per row of a free node
//                assembles that row of the node's diagonal block, of its block towards node k + 1 and of g over the node's edges in the
//                stated order.
//     trial      segments are independent: one wave per segment at a time walks it upward; per node the lanes cover the 6 x 19 panel
//                [D | U | F | y] (diagonal block, right neighbour, left bounding separator, right-hand side) in LDS, six scaled-row /
//                update steps, and the 78 products that the next node and the bounding separators receive.  The separator system is
//                assembled in the workspace (one owner per entry; the loop blocks by 36 threads in ascending record index), factorised
//                right-looking column by column by the whole workgroup (the scaled column staged in LDS, the trailing update on the
//                VALU), solved forward and backward likewise;  the segments are back-substituted by their waves;  the poses move (se3_retract,
//                solver_math.h);  the cost at the candidate is one more pass over the edges.
//                Every thread carries the scalars of the schedule (lambda, c, trials) itself, from values broadcast through LDS, so
//                every branch of the loops is uniform.  A rejected trial changes only lambda: the same H and g are factorised again.
//   k_pg_odometry, k_pg_loops   the two gather stages, one thread per slot / record.
// No local array is indexed by a run-time value; plain vector stores only: profiles/pg_solve_resource_usage.txt.
#include "../../include/sship.h"
#include "kernels.h"
#include "solver_math.h"

namespace sship {

namespace {

constexpr int kPgThreads = 256;
constexpr int kPgEdge = 80;      // doubles per linearised edge: r~ 6, w, rho, J~_i 36, J~_j 36
constexpr int kPgFac = 114;      // doubles per eliminated node: the 6 x 19 panel [R | U' | F' | y']
constexpr int kPgSeg = 120;      // doubles per segment: F'^T F' 36, F'^T y' 6, U'^T U' 36, U'^T F' 36, U'^T y' 6 (of its last node)
constexpr int kPgPanelLd = 20;
constexpr int kPgMaxOrder = 12 * kPgMaxLoops;

// the lanes of one wave exchange data through LDS: order this wave's LDS traffic
__device__ __forceinline__ void pg_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the coefficients of the rule at x = theta^2 (include/sship.h)
struct PgCoef { double A, B, C, D, C2, C3; };
__device__ __forceinline__ PgCoef pg_coef(double x) {
  PgCoef k;
  if (x < 1e-2) {
    k.A = 1.0 - x / 6.0 * (1.0 - x / 20.0 * (1.0 - x / 42.0 * (1.0 - x / 72.0)));
    k.B = 0.5 * (1.0 - x / 12.0 * (1.0 - x / 30.0 * (1.0 - x / 56.0 * (1.0 - x / 90.0))));
    k.C = (1.0 - x / 20.0 * (1.0 - x / 42.0 * (1.0 - x / 72.0 * (1.0 - x / 110.0)))) / 6.0;
    k.D = 1.0 / 12.0 + x / 720.0 + x * x / 30240.0 + x * x * x / 1209600.0;
    k.C2 = (1.0 - x / 30.0 * (1.0 - x / 56.0 * (1.0 - x / 90.0))) / 24.0;
    k.C3 = 1.0 / 120.0 - x / 2520.0 + x * x / 120960.0 - x * x * x / 9979200.0;
  } else {
    const double th = sqrt(x), s = sin(th), c = cos(th), sh = sin(0.5 * th);
    k.A = s / th;
    k.B = 2.0 * sh * sh / x;
    k.C = (th - s) / (x * th);
    k.D = (1.0 - k.A / (2.0 * k.B)) / x;
    k.C2 = (x + 2.0 * c - 2.0) / (2.0 * x * x);
    k.C3 = (2.0 * th - 3.0 * s + th * c) / (2.0 * x * x * th);
  }
  return k;
}

__device__ __forceinline__ void pg_mul(const double* a, const double* b, double* o) {  // 3x3, o = a b
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
__device__ __forceinline__ void pg_skew(double x, double y, double z, double* o) {
  o[0] = 0.0; o[1] = -z; o[2] = y; o[3] = z; o[4] = 0.0; o[5] = -x; o[6] = -y; o[7] = x; o[8] = 0.0;
}

// r = Log(Z^-1 Ti^-1 Tj), unwhitened; X = Ti^-1 Tj = [Rx | tx] is kept for the Jacobians
struct PgRes { double r[6], Rx[9], tx[3]; };
__device__ __forceinline__ void pg_residual(const double* Ti, const double* Tj, const double* Z, PgRes& o) {
  double d[3], u[3], RE[9], tE[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) d[m] = Tj[4 * m + 3] - Ti[4 * m + 3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) o.Rx[3 * a + b] = Ti[a] * Tj[b] + Ti[4 + a] * Tj[4 + b] + Ti[8 + a] * Tj[8 + b];
    o.tx[a] = Ti[a] * d[0] + Ti[4 + a] * d[1] + Ti[8 + a] * d[2];
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) u[m] = o.tx[m] - Z[4 * m + 3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) RE[3 * a + b] = Z[a] * o.Rx[b] + Z[4 + a] * o.Rx[3 + b] + Z[8 + a] * o.Rx[6 + b];
    tE[a] = Z[a] * u[0] + Z[4 + a] * u[1] + Z[8 + a] * u[2];
  }
  const double a0 = 0.5 * (RE[7] - RE[5]), a1 = 0.5 * (RE[2] - RE[6]), a2 = 0.5 * (RE[3] - RE[1]);
  const double s = sqrt(a0 * a0 + a1 * a1 + a2 * a2), c = 0.5 * (RE[0] + RE[4] + RE[8] - 1.0);
  const double th = atan2(s, c), x = th * th;
  const PgCoef k = pg_coef(x);
  const double f = x < 1e-2 ? 1.0 / k.A : th / s;
  const double w0 = f * a0, w1 = f * a1, w2 = f * a2;
  const double p0 = w1 * tE[2] - w2 * tE[1], p1 = w2 * tE[0] - w0 * tE[2], p2 = w0 * tE[1] - w1 * tE[0];   // omega x t
  const double q0 = w1 * p2 - w2 * p1, q1 = w2 * p0 - w0 * p2, q2 = w0 * p1 - w1 * p0;                     // omega x (omega x t)
  o.r[0] = w0; o.r[1] = w1; o.r[2] = w2;
  o.r[3] = tE[0] - 0.5 * p0 + k.D * q0;
  o.r[4] = tE[1] - 0.5 * p1 + k.D * q1;
  o.r[5] = tE[2] - 0.5 * p2 + k.D * q2;
}

// whitened residual, weight and rho of an edge from its raw residual
struct PgW { double rw[6], e2, w, rho; };
__device__ __forceinline__ PgW pg_whiten(const double* r, const double* sg, double k2) {
  PgW o;
  o.e2 = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) { o.rw[a] = r[a] / sg[a]; o.e2 += o.rw[a] * o.rw[a]; }
  const double e = sqrt(o.e2), k = sqrt(fmax(k2, 0.0));
  const bool quad = !(k2 > 0.0) || e <= k;
  o.w = quad ? 1.0 : k / e;
  o.rho = quad ? 0.5 * o.e2 : k * e - 0.5 * k2;
  return o;
}

// the two whitened Jacobians (row-major 6x6) of an edge to global memory
__device__ __forceinline__ void pg_jacobians(const PgRes& o, const double* sg, double* Ji, double* Jj) {
  const double wx = -o.r[0], wy = -o.r[1], wz = -o.r[2];
  const PgCoef k = pg_coef(wx * wx + wy * wy + wz * wz);
  double P[9], R[9], PP[9], Ai[9], PR[9], RP[9], PRP[9], PPR[9], RPP[9], PRPP[9], PPRP[9], Q[9], T1[9], Bl[9];
  pg_skew(wx, wy, wz, P);
  pg_skew(-o.r[3], -o.r[4], -o.r[5], R);
  pg_mul(P, P, PP);
  pg_mul(P, R, PR); pg_mul(R, P, RP); pg_mul(PR, P, PRP); pg_mul(P, PR, PPR); pg_mul(RP, P, RPP); pg_mul(PRP, P, PRPP); pg_mul(P, PRP, PPRP);
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    Ai[i] = ((i % 4) == 0 ? 1.0 : 0.0) - 0.5 * P[i] + k.D * PP[i];
    Q[i] = 0.5 * R[i] + k.C * (PR[i] + RP[i] + PRP[i]) + k.C2 * (PPR[i] + RPP[i] - 3.0 * PRP[i]) + k.C3 * (PRPP[i] + PPRP[i]);
  }
  pg_mul(Ai, Q, T1);
  pg_mul(T1, Ai, Bl);
#pragma unroll
  for (int i = 0; i < 9; ++i) Bl[i] = -Bl[i];
  // Ad(Tj^-1 Ti): Ra = Rx^T, ta = -Rx^T tx
  double Ra[9], Ka[9], S[9], ta[3], AR[9], BR[9], AK[9];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) Ra[3 * a + b] = o.Rx[3 * b + a];
    ta[a] = -(o.Rx[a] * o.tx[0] + o.Rx[3 + a] * o.tx[1] + o.Rx[6 + a] * o.tx[2]);
  }
  pg_skew(ta[0], ta[1], ta[2], S);
  pg_mul(S, Ra, Ka);
  pg_mul(Ai, Ra, AR); pg_mul(Bl, Ra, BR); pg_mul(Ai, Ka, AK);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double s0 = 1.0 / sg[a], s1 = 1.0 / sg[3 + a];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      Jj[6 * a + b] = Ai[3 * a + b] * s0;          Jj[6 * a + 3 + b] = 0.0;
      Jj[6 * (3 + a) + b] = Bl[3 * a + b] * s1;    Jj[6 * (3 + a) + 3 + b] = Ai[3 * a + b] * s1;
      Ji[6 * a + b] = -AR[3 * a + b] * s0;         Ji[6 * a + 3 + b] = 0.0;
      Ji[6 * (3 + a) + b] = -(BR[3 * a + b] + AK[3 * a + b]) * s1;
      Ji[6 * (3 + a) + 3 + b] = -AR[3 * a + b] * s1;
    }
  }
}

// the workspace slice of one resident workgroup (pg_workspace_bytes)
struct PgWs {
  double *edge, *T, *Tn, *D, *U, *g, *fac, *delta, *seg, *S;
  int *sepflag, *sepidx, *oflag, *seplist, *segL, *segR, *segstart, *segend;
  char* end;   // one past the slice's last byte
};
__device__ __host__ __forceinline__ int pg_max_sep(int N, int L) { return 2 * L < N - 1 ? 2 * L : N - 1; }
__device__ __host__ __forceinline__ PgWs pg_slice(char* base, int N, int L) {
  PgWs w;
  const size_t S = (size_t)pg_max_sep(N, L);
  double* d = reinterpret_cast<double*>(base);
  w.edge = d; d += (size_t)kPgEdge * (N - 1 + L);
  w.T = d; d += 12 * (size_t)N;
  w.Tn = d; d += 12 * (size_t)N;
  w.D = d; d += 36 * (size_t)N;
  w.U = d; d += 36 * (size_t)N;
  w.g = d; d += 6 * (size_t)N;
  w.fac = d; d += (size_t)kPgFac * N;
  w.delta = d; d += 6 * (size_t)N;
  w.seg = d; d += (size_t)kPgSeg * (S + 1);
  w.S = d; d += 36 * S * S;
  int* i = reinterpret_cast<int*>(d);
  w.sepflag = i; i += N;
  w.sepidx = i; i += N;
  w.oflag = i; i += N;
  w.seplist = i; i += S;
  w.segL = i; i += S;
  w.segR = i; i += S;
  w.segstart = i; i += S + 1;
  w.segend = i; i += S + 1;
  w.end = reinterpret_cast<char*>(i);
  return w;
}

}  // namespace

size_t pg_workspace_bytes(int N, int L) {   // the extent of pg_slice's own layout, which include/sship.h states as a formula
  const size_t b = static_cast<size_t>(pg_slice(nullptr, N, L).end - static_cast<char*>(nullptr));
  return (b + 15) / 16 * 16;
}

__global__ __launch_bounds__(kPgThreads) void k_pg_solve(const int32_t* __restrict__ n_nodes_dev, const double* __restrict__ pose0,
                                                        const double* __restrict__ odom_z, const double* __restrict__ odom_sigma,
                                                        const int32_t* __restrict__ loop_ij, const double* __restrict__ loop_z,
                                                        const double* __restrict__ loop_sigma, const double* __restrict__ loop_k2,
                                                        const uint8_t* __restrict__ loop_enable, int N, int L, int graphs, PgK P,
                                                        char* __restrict__ ws_base, size_t ws_stride, double* __restrict__ pose,
                                                        int32_t* __restrict__ stats, double* __restrict__ cost, double* __restrict__ loop_chi2) {
  __shared__ double s_col[kPgMaxOrder];        // the scaled column of the separator factorisation
  __shared__ double s_rhs[kPgMaxOrder];        // the separator right-hand side, then its solution
  __shared__ double s_P[4][6 * kPgPanelLd];    // per wave: the panel of the node being eliminated
  __shared__ double s_Q[4][80];                // per wave: what the next node receives: U'^T U' 36, U'^T F' 36, U'^T y' 6
  __shared__ double s_dn[4][8];                // per wave: delta of the node above during back-substitution
  __shared__ double s_red[4];
  __shared__ double s_val;
  __shared__ int s_li[kPgMaxLoops], s_lj[kPgMaxLoops];
  __shared__ int s_lstat[kPgMaxLoops], s_lpres[kPgMaxLoops];   // present before / after the rejection loop's drops
  __shared__ int s_flag, s_nodom, s_ns, s_nseg, s_top;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PgWs ws = pg_slice(ws_base + (size_t)blockIdx.x * ws_stride, N, L);
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);

  for (int gr = blockIdx.x; gr < graphs; gr += gridDim.x) {
    __syncthreads();  // the previous graph's last readers of LDS
    const double* p0 = pose0 + (size_t)gr * N * 12;
    const double* oz = odom_z + (size_t)gr * (N - 1) * 12;
    const double* osg = odom_sigma ? odom_sigma + (size_t)gr * (N - 1) * 6 : nullptr;
    const int32_t* lij = L ? loop_ij + (size_t)gr * L * 2 : nullptr;
    const double* lz = L ? loop_z + (size_t)gr * L * 12 : nullptr;
    const double* lsg = L ? loop_sigma + (size_t)gr * L * 6 : nullptr;
    const double* lk2 = L ? loop_k2 + (size_t)gr * L : nullptr;
    const uint8_t* len = (L && loop_enable) ? loop_enable + (size_t)gr * L : nullptr;
    double* gpose = pose + (size_t)gr * N * 12;
    const int n = n_nodes_dev ? min(max(n_nodes_dev[gr], 0), N) : N;
    const int n_e = max(n - 1, 0) + L;   // the edge index space: odometry slots k < n - 1, then the loop records

    // ---- setup: the state, presence ----
    if (tid == 0) { s_flag = 0; s_nodom = 0; }
    __syncthreads();
    for (int i = tid; i < n * 12; i += kPgThreads) {
      const double t = p0[i];
      ws.T[i] = t; ws.Tn[i] = t;
      if (!solver_finite(t)) atomicOr(&s_flag, 1);
    }
    {
      int cnt = 0;
      for (int k = tid; k < n - 1; k += kPgThreads) {
        bool ok = true;
        for (int i = 0; i < 12; ++i) ok = ok && solver_finite(oz[(size_t)k * 12 + i]);
        if (osg)
          for (int i = 0; i < 6; ++i) { const double sg = osg[(size_t)k * 6 + i]; ok = ok && solver_finite(sg) && sg > 0.0; }
        ws.oflag[k] = ok ? 1 : 0;
        cnt += ok ? 1 : 0;
      }
      if (cnt) atomicAdd(&s_nodom, cnt);
    }
    for (int l = tid; l < L; l += kPgThreads) {
      const int i = lij[2 * l], j = lij[2 * l + 1];
      bool ok = (unsigned)i < (unsigned)n && (unsigned)j < (unsigned)n && i != j && (!len || len[l] != 0) && solver_finite(lk2[l]);
      for (int q = 0; q < 12; ++q) ok = ok && solver_finite(lz[(size_t)l * 12 + q]);
      for (int q = 0; q < 6; ++q) { const double sg = lsg[(size_t)l * 6 + q]; ok = ok && solver_finite(sg) && sg > 0.0; }
      s_li[l] = i; s_lj[l] = j; s_lstat[l] = ok ? 1 : 0; s_lpres[l] = ok ? 1 : 0;
    }
    __syncthreads();
    const bool bad_input = s_flag != 0;
    const int n_odom = s_nodom;
    int n_loops = 0;
    for (int l = 0; l < L; ++l) n_loops += s_lstat[l];
    int status = SSHIP_PG_CONVERGED, trials = 0, dropped = 0;
    double c = 0.0, c_init = 0.0;
    if (bad_input) status = SSHIP_PG_BAD_INPUT;
    else if (n < 2 || n_odom + n_loops == 0) status = SSHIP_PG_TOO_FEW;
    const bool early = status != SSHIP_PG_CONVERGED;

    // one edge of the index space at the poses Ts: false if absent
    auto edge_at = [&](int e, const double* Ts, PgRes& res, double* sg, double& k2) -> bool {
      int i, j;
      const double* Z;
      if (e < n - 1) {
        if (!ws.oflag[e]) return false;
        i = e; j = e + 1; Z = oz + (size_t)e * 12; k2 = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) sg[a] = osg ? osg[(size_t)e * 6 + a] : (a < 3 ? P.odom_sigma_rot : P.odom_sigma_trans);
      } else {
        const int l = e - (n - 1);
        if (!s_lpres[l]) return false;
        i = s_li[l]; j = s_lj[l]; Z = lz + (size_t)l * 12; k2 = lk2[l];
#pragma unroll
        for (int a = 0; a < 6; ++a) sg[a] = lsg[(size_t)l * 6 + a];
      }
      pg_residual(Ts + (size_t)i * 12, Ts + (size_t)j * 12, Z, res);
      return true;
    };
    // where edge e of the index space is kept in the workspace
    auto edge_slot = [&](int e) -> double* { return ws.edge + (size_t)kPgEdge * (e < n - 1 ? e : e - (n - 1) + (N - 1)); };

    // the cost at Ts: every thread over its edges in index order, a butterfly, the waves in order -> returned to every thread
    auto cost_at = [&](const double* Ts) -> double {
      double acc = 0.0;
      for (int e = tid; e < n_e; e += kPgThreads) {
        PgRes res; double sg[6], k2;
        if (!edge_at(e, Ts, res, sg, k2)) continue;
        acc += pg_whiten(res.r, sg, k2).rho;
      }
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
      __syncthreads();  // s_red, s_val free
      if (lane == 0) s_red[wave] = acc;
      __syncthreads();
      if (tid == 0) s_val = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
      __syncthreads();
      return s_val;
    };

    // r~, w, J~ of every present edge, then D_k, U_k = H[k][k + 1] and g_k of every free node, at the state ws.T
    auto linearise = [&]() {
      for (int e = tid; e < n_e; e += kPgThreads) {
        PgRes res; double sg[6], k2;
        if (!edge_at(e, ws.T, res, sg, k2)) continue;
        const PgW w = pg_whiten(res.r, sg, k2);
        double* E = edge_slot(e);
#pragma unroll
        for (int a = 0; a < 6; ++a) E[a] = w.rw[a];
        E[6] = w.w; E[7] = w.rho;
        pg_jacobians(res, sg, E + 8, E + 44);
      }
      __syncthreads();
      for (int t = tid; t < 6 * (n - 1); t += kPgThreads) {
        const int k = 1 + t / 6, a = t % 6;
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, u[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ga = 0.0;
        auto add = [&](const double* E, const double* J) {
          const double w = E[6];
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            const double ja = w * J[6 * r + a];
#pragma unroll
            for (int b = 0; b < 6; ++b) acc[b] += ja * J[6 * r + b];
            ga += ja * E[r];
          }
        };
        if (ws.oflag[k - 1]) { const double* E = edge_slot(k - 1); add(E, E + 44); }
        if (k < n - 1 && ws.oflag[k]) {
          const double* E = edge_slot(k);
          add(E, E + 8);
          const double w = E[6];
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            const double ja = w * E[8 + 6 * r + a];
#pragma unroll
            for (int b = 0; b < 6; ++b) u[b] += ja * E[44 + 6 * r + b];
          }
        }
        for (int l = 0; l < L; ++l) {
          if (!s_lpres[l]) continue;
          const double* E = ws.edge + (size_t)kPgEdge * (N - 1 + l);
          if (s_li[l] == k) add(E, E + 8);
          else if (s_lj[l] == k) add(E, E + 44);
        }
#pragma unroll
        for (int b = 0; b < 6; ++b) { ws.D[(size_t)k * 36 + a * 6 + b] = acc[b]; ws.U[(size_t)k * 36 + a * 6 + b] = u[b]; }
        ws.g[(size_t)k * 6 + a] = ga;
      }
      __syncthreads();
    };

    if (!early) {
      for (;;) {  // the rejection loop: one attempt per pass
        // ---- the structure of this attempt: separators and segment starts in ascending node index ----
        for (int k = tid; k < n; k += kPgThreads) { ws.sepflag[k] = 0; ws.sepidx[k] = -1; }
        __syncthreads();
        for (int l = tid; l < L; l += kPgThreads)
          if (s_lpres[l]) {
            if (s_li[l] > 0) ws.sepflag[s_li[l]] = 1;
            if (s_lj[l] > 0) ws.sepflag[s_lj[l]] = 1;
          }
        __syncthreads();
        if (wave == 0) {
          int nsep = 0, nsg = 0;
          for (int k0 = 1; k0 < n; k0 += 64) {
            const int k = k0 + lane;
            const bool sep = k < n && ws.sepflag[k] != 0;
            const bool start = k < n && !sep && (k == 1 || ws.sepflag[k - 1] != 0);
            const unsigned long long bs = __ballot(sep), bg = __ballot(start);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (sep) { const int o = nsep + __popcll(bs & below); ws.sepidx[k] = o; ws.seplist[o] = k; }
            if (start) ws.segstart[nsg + __popcll(bg & below)] = k;
            nsep += __popcll(bs); nsg += __popcll(bg);
          }
          if (lane == 0) { s_ns = nsep; s_nseg = nsg; }
        }
        __syncthreads();
        const int ns = s_ns, nseg = s_nseg, m = 6 * ns;
        for (int s = tid; s < ns; s += kPgThreads) { ws.segL[s] = -1; ws.segR[s] = -1; }
        for (int i = tid; i < n * 12; i += kPgThreads) { const double t = p0[i]; ws.T[i] = t; ws.Tn[i] = t; }
        __syncthreads();

        double lambda = P.lambda0;
        int att_trials = 0;
        linearise();
        c = cost_at(ws.T);
        if (dropped == 0) c_init = c;
        for (;;) {
          if (att_trials >= P.max_iterations) { status = SSHIP_PG_ITER_CAP; break; }
          ++att_trials; ++trials;
          if (tid == 0) s_flag = 0;
          __syncthreads();
          // ---- the segments, one wave each at a time, from the lowest node upward ----
          for (int sg = wave; sg < nseg; sg += 4) {
            double* Pn = s_P[wave];
            double* Qn = s_Q[wave];
            const int a = ws.segstart[sg];
            const int left = a - 1 >= 1 ? ws.sepidx[a - 1] : -1;
            double accL = 0.0;   // lanes 0..35: F'^T F' summed over the segment, lanes 36..41: F'^T y'
            bool fail = false;
            for (int e = lane; e < 80; e += 64) Qn[e] = 0.0;
            int k = a;
            for (;;) {
              pg_wave_sync();
              for (int e = lane; e < 6 * 19; e += 64) {
                const int r = e / 19, cc = e % 19;
                double v;
                if (cc < 6) v = ws.D[(size_t)k * 36 + r * 6 + cc] + (r == cc ? lambda : 0.0) - Qn[r * 6 + cc];
                else if (cc < 12) v = k + 1 < n ? ws.U[(size_t)k * 36 + r * 6 + cc - 6] : 0.0;
                else if (cc < 18) v = k == a ? (left >= 0 ? ws.U[(size_t)(a - 1) * 36 + (cc - 12) * 6 + r] : 0.0) : -Qn[36 + r * 6 + cc - 12];
                else v = -ws.g[(size_t)k * 6 + r] - Qn[72 + r];
                Pn[r * kPgPanelLd + cc] = v;
              }
              pg_wave_sync();
#pragma unroll
              for (int j = 0; j < 6; ++j) {
                const double d = Pn[j * kPgPanelLd + j];
                if (!(d > 0.0)) fail = true;
                const double il = 1.0 / sqrt(d);
                pg_wave_sync();
                if (lane >= j && lane < 19) Pn[j * kPgPanelLd + lane] *= il;
                pg_wave_sync();
                for (int e = lane; e < (5 - j) * 19; e += 64) {
                  const int i = j + 1 + e / 19, cc = e % 19;
                  if (cc > j) Pn[i * kPgPanelLd + cc] -= Pn[j * kPgPanelLd + i] * Pn[j * kPgPanelLd + cc];
                }
                pg_wave_sync();
              }
              for (int e = lane; e < kPgFac; e += 64) ws.fac[(size_t)k * kPgFac + e] = Pn[(e / 19) * kPgPanelLd + e % 19];
              for (int e = lane; e < 78; e += 64) {
                const int p = e < 72 ? (e % 36) / 6 : e - 72;
                const int col = e < 36 ? 6 + e % 6 : (e < 72 ? 12 + e % 6 : 18);
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < 6; ++r) v += Pn[r * kPgPanelLd + 6 + p] * Pn[r * kPgPanelLd + col];
                Qn[e] = v;
              }
              if (lane < 42) {
                const int p = lane < 36 ? lane / 6 : lane - 36;
                const int col = lane < 36 ? 12 + lane % 6 : 18;
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < 6; ++r) v += Pn[r * kPgPanelLd + 12 + p] * Pn[r * kPgPanelLd + col];
                accL += v;
              }
              if (k + 1 >= n || ws.sepflag[k + 1] != 0) break;
              ++k;
            }
            pg_wave_sync();
            const int right = k + 1 < n ? ws.sepidx[k + 1] : -1;
            if (lane < 42) ws.seg[(size_t)sg * kPgSeg + lane] = accL;
            for (int e = lane; e < 78; e += 64) ws.seg[(size_t)sg * kPgSeg + 42 + e] = Qn[e];
            if (lane == 0) {
              ws.segend[sg] = k;
              if (left >= 0) ws.segR[left] = sg;
              if (right >= 0) ws.segL[right] = sg;
              if (fail) atomicOr(&s_flag, 1);
            }
          }
          __syncthreads();
          bool ok = s_flag == 0;
          __syncthreads();  // s_flag is cleared again at the top of the next trial
          // ---- the separator system: S (lower triangle, row-major, order m) and its right-hand side ----
          if (ok && m > 0) {
            for (size_t e = tid; e < (size_t)m * m; e += kPgThreads) ws.S[e] = 0.0;
            __syncthreads();
            for (int t = tid; t < ns * 42; t += kPgThreads) {
              const int s = t / 42, e = t % 42, node = ws.seplist[s], sl = ws.segL[s], sr = ws.segR[s];
              if (e < 36) {
                const int r = e / 6, cc = e % 6;
                double v = ws.D[(size_t)node * 36 + e] + (r == cc ? lambda : 0.0);
                if (sl >= 0) v -= ws.seg[(size_t)sl * kPgSeg + 42 + e];
                if (sr >= 0) v -= ws.seg[(size_t)sr * kPgSeg + e];
                ws.S[(size_t)(6 * s + r) * m + 6 * s + cc] = v;
              } else {
                const int p = e - 36;
                double v = -ws.g[(size_t)node * 6 + p];
                if (sl >= 0) v -= ws.seg[(size_t)sl * kPgSeg + 42 + 72 + p];
                if (sr >= 0) v -= ws.seg[(size_t)sr * kPgSeg + 36 + p];
                s_rhs[6 * s + p] = v;
              }
            }
            for (int t = tid; t < (ns - 1) * 36; t += kPgThreads) {   // two separators that are neighbours in the chain
              const int s = t / 36, r = (t % 36) / 6, cc = t % 6, node = ws.seplist[s];
              if (ws.seplist[s + 1] == node + 1) ws.S[(size_t)(6 * (s + 1) + r) * m + 6 * s + cc] = ws.U[(size_t)node * 36 + cc * 6 + r];
            }
            for (int t = tid; t < nseg * 36; t += kPgThreads) {       // the fill between the two bounds of a segment
              const int sg = t / 36, p = (t % 36) / 6, q = t % 6, a = ws.segstart[sg], b = ws.segend[sg];
              if (a - 1 >= 1 && b + 1 < n)
                ws.S[(size_t)(6 * ws.sepidx[b + 1] + p) * m + 6 * ws.sepidx[a - 1] + q] = -ws.seg[(size_t)sg * kPgSeg + 78 + p * 6 + q];
            }
            __syncthreads();
            if (tid < 36) {   // the loops' blocks, every entry in ascending record index
              const int p = tid / 6, q = tid % 6;
              for (int l = 0; l < L; ++l) {
                if (!s_lpres[l] || s_li[l] == 0 || s_lj[l] == 0) continue;
                const double* E = ws.edge + (size_t)kPgEdge * (N - 1 + l);
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < 6; ++r) v += E[6] * E[8 + 6 * r + p] * E[44 + 6 * r + q];   // (w J_i^T J_j)[p][q]
                const int si = ws.sepidx[s_li[l]], sj = ws.sepidx[s_lj[l]];
                if (si > sj) ws.S[(size_t)(6 * si + p) * m + 6 * sj + q] += v;
                else ws.S[(size_t)(6 * sj + q) * m + 6 * si + p] += v;
              }
            }
            __syncthreads();
            // ---- Cholesky of S in place (lower), right-looking, column by column ----
            for (int j = 0; j < m; ++j) {
              const double d = ws.S[(size_t)j * m + j];
              if (!(d > 0.0)) { ok = false; break; }  // uniform: every thread read the same value
              const double lj = sqrt(d), il = 1.0 / lj;
              __syncthreads();   // every thread has read the pivot; s_col free
              for (int i = j + tid; i < m; i += kPgThreads) {
                const double v = i == j ? lj : ws.S[(size_t)i * m + j] * il;
                ws.S[(size_t)i * m + j] = v; s_col[i] = v;
              }
              __syncthreads();
              for (int i = j + 1 + (tid >> 4); i < m; i += 16) {
                const double ci = s_col[i];
                for (int q = j + 1 + (tid & 15); q <= i; q += 16) ws.S[(size_t)i * m + q] -= ci * s_col[q];
              }
              __syncthreads();
            }
            if (ok) {  // L y = b, L^T x = y, in place in s_rhs
              for (int j = 0; j < m; ++j) {
                __syncthreads();
                const double yj = s_rhs[j] / ws.S[(size_t)j * m + j];
                __syncthreads();
                if (tid == 0) s_rhs[j] = yj;
                for (int i = j + 1 + tid; i < m; i += kPgThreads) s_rhs[i] -= ws.S[(size_t)i * m + j] * yj;
              }
              for (int j = m - 1; j >= 0; --j) {
                __syncthreads();
                const double xj = s_rhs[j] / ws.S[(size_t)j * m + j];
                __syncthreads();
                if (tid == 0) s_rhs[j] = xj;
                for (int i = tid; i < j; i += kPgThreads) s_rhs[i] -= ws.S[(size_t)j * m + i] * xj;
              }
              __syncthreads();
              for (int t = tid; t < m; t += kPgThreads) ws.delta[(size_t)ws.seplist[t / 6] * 6 + t % 6] = s_rhs[t];
            }
          }
          __syncthreads();
          if (ok) {
            // ---- the segments again, from the highest node downward: R delta_k = y' - U' delta_{k+1} - F' delta_left ----
            for (int sg = wave; sg < nseg; sg += 4) {
              double* Pn = s_P[wave];
              double* dn = s_dn[wave];
              const int a = ws.segstart[sg], b = ws.segend[sg];
              const bool has_left = a - 1 >= 1;
              if (lane < 6) dn[lane] = b + 1 < n ? ws.delta[(size_t)(b + 1) * 6 + lane] : 0.0;
              for (int k = b; k >= a; --k) {
                const double* F = ws.fac + (size_t)k * kPgFac;
                pg_wave_sync();
                if (lane < 6) {
                  double t = F[lane * 19 + 18];
#pragma unroll
                  for (int cc = 0; cc < 6; ++cc) t -= F[lane * 19 + 6 + cc] * dn[cc];
                  if (has_left) {
#pragma unroll
                    for (int cc = 0; cc < 6; ++cc) t -= F[lane * 19 + 12 + cc] * ws.delta[(size_t)(a - 1) * 6 + cc];
                  }
                  Pn[lane * kPgPanelLd + 6] = t;
                }
                if (lane >= 8 && lane < 44) Pn[((lane - 8) / 6) * kPgPanelLd + (lane - 8) % 6] = F[((lane - 8) / 6) * 19 + (lane - 8) % 6];
                pg_wave_sync();
                if (lane == 0) {
                  double x[6];
#pragma unroll
                  for (int r = 5; r >= 0; --r) {
                    double t = Pn[r * kPgPanelLd + 6];
#pragma unroll
                    for (int cc = r + 1; cc < 6; ++cc) t -= Pn[r * kPgPanelLd + cc] * x[cc];
                    x[r] = t / Pn[r * kPgPanelLd + r];
                  }
#pragma unroll
                  for (int r = 0; r < 6; ++r) { dn[r] = x[r]; ws.delta[(size_t)k * 6 + r] = x[r]; }
                }
              }
            }
            __syncthreads();
            // ---- the candidate ----
            for (int k = 1 + tid; k < n; k += kPgThreads) {
              double delta[6], Tl[12], Tn[12];
#pragma unroll
              for (int i = 0; i < 6; ++i) delta[i] = ws.delta[(size_t)k * 6 + i];
#pragma unroll
              for (int i = 0; i < 12; ++i) Tl[i] = ws.T[(size_t)k * 12 + i];
              se3_retract(Tl, delta, Tn);
#pragma unroll
              for (int i = 0; i < 12; ++i) ws.Tn[(size_t)k * 12 + i] = Tn[i];
            }
            __syncthreads();
            const double cn = cost_at(ws.Tn);
            const bool conv = solver_finite(cn) && fabs(c - cn) <= fmax(P.abs_tol, P.rel_tol * c);
            if (conv || cn < c) {  // the candidate becomes the state
              for (int i = 12 + tid; i < n * 12; i += kPgThreads) ws.T[i] = ws.Tn[i];
              c = cn;
              __syncthreads();
              if (conv) { status = SSHIP_PG_CONVERGED; break; }
              lambda /= 10.0;
              linearise();
              continue;
            }
          }
          lambda *= 10.0;
          if (lambda > P.lambda_max) { status = SSHIP_PG_STALLED; break; }
        }
        // ---- sane?  otherwise the present loop with the highest record index goes ----
        __syncthreads();
        if (tid == 0) { s_flag = 0; s_top = -1; }
        __syncthreads();
        for (int k = tid; k < n; k += kPgThreads) {
          bool ok = true;
          for (int i = 0; i < 12; ++i) ok = ok && solver_finite(ws.T[(size_t)k * 12 + i]);
          const double tx = ws.T[(size_t)k * 12 + 3], ty = ws.T[(size_t)k * 12 + 7], tz = ws.T[(size_t)k * 12 + 11];
          ok = ok && sqrt(tx * tx + ty * ty + tz * tz) <= P.max_translation;
          if (!ok) atomicOr(&s_flag, 1);
        }
        for (int l = tid; l < L; l += kPgThreads)
          if (s_lpres[l]) atomicMax(&s_top, l);
        __syncthreads();
        const bool sane = s_flag == 0;
        const int top = s_top;
        __syncthreads();
        if (sane) break;
        if (top < 0) { status = SSHIP_PG_DIVERGED; break; }
        if (tid == 0) s_lpres[top] = 0;
        ++dropped; --n_loops;
        __syncthreads();
      }
    }

    // ---- outputs: every entry written ----
    __syncthreads();
    const bool keep_in = early || status == SSHIP_PG_DIVERGED;
    for (int i = tid; i < N * 12; i += kPgThreads) {
      const int k = i / 12;
      gpose[i] = (keep_in || k == 0 || k >= n) ? p0[i] : ws.T[i];
    }
    if (loop_chi2) {
      double* gchi = loop_chi2 + (size_t)gr * L;
      for (int l = tid; l < L; l += kPgThreads) {
        double v = qnan;
        if (!early && s_lpres[l]) {
          PgRes res; double sg[6], k2;
          edge_at(n - 1 + l, ws.T, res, sg, k2);
          v = pg_whiten(res.r, sg, k2).e2;
        }
        gchi[l] = v;
      }
    }
    if (tid == 0) {
      stats[gr * 4 + 0] = n_odom + n_loops; stats[gr * 4 + 1] = dropped; stats[gr * 4 + 2] = trials; stats[gr * 4 + 3] = status;
      cost[gr * 2 + 0] = early ? 0.0 : c_init; cost[gr * 2 + 1] = early ? 0.0 : c;
    }
  }
}

// odom_z[g, k] = T_k^-1 T_{k+1}; products and sums rounded one by one, so that the stage can be restated bit for bit
__global__ __launch_bounds__(256) void k_pg_odometry(const double* __restrict__ pose, int N, long long total, double* __restrict__ odom_z) {
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long long g = t / (N - 1), k = t % (N - 1);
  const double* A = pose + (g * N + k) * 12;
  const double* B = A + 12;
  double* Z = odom_z + t * 12;
  const double d0 = B[3] - A[3], d1 = B[7] - A[7], d2 = B[11] - A[11];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) Z[4 * a + b] = (A[a] * B[b] + A[4 + a] * B[4 + b]) + A[8 + a] * B[8 + b];
    Z[4 * a + 3] = (A[a] * d0 + A[4 + a] * d1) + A[8 + a] * d2;
  }
}

// loop records from the pose solver's results (include/sship.h)
__global__ __launch_bounds__(256) void k_pg_loops(const int32_t* __restrict__ from, const int32_t* __restrict__ to,
                                                 const double* __restrict__ pose, const int32_t* __restrict__ stats, int pairs, int min_inliers,
                                                 double noise_base, int32_t* __restrict__ loop_ij, double* __restrict__ loop_z,
                                                 double* __restrict__ loop_sigma, double* __restrict__ loop_k2, uint8_t* __restrict__ loop_enable) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= pairs) return;
  const int n_obs = stats[4 * p], n_in = stats[4 * p + 1], st = stats[4 * p + 3];
  bool ok = n_obs >= min_inliers && n_in >= min_inliers && st != SSHIP_POSE_TOO_FEW && st != SSHIP_POSE_BAD_INPUT;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const double v = pose[(size_t)p * 12 + i];
    ok = ok && solver_finite(v);
    loop_z[(size_t)p * 12 + i] = v;
  }
  double sr = 0.02, st_ = 0.20;
  if (ok) {
    const double s = noise_base / sqrt((double)n_in);
    sr = fmax(s, 0.02); st_ = fmax(s, 0.20);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) loop_sigma[(size_t)p * 6 + i] = i < 3 ? sr : st_;
  loop_ij[2 * p] = from[p]; loop_ij[2 * p + 1] = to[p];
  loop_k2[p] = 7.815;
  loop_enable[p] = ok ? 1 : 0;
}

void launch_pg_solve(const int32_t* n_nodes, const double* pose0, const double* odom_z, const double* odom_sigma, const int32_t* loop_ij,
                     const double* loop_z, const double* loop_sigma, const double* loop_k2, const uint8_t* loop_enable, int N, int L, int graphs,
                     const PgK& k, void* ws, double* pose, int32_t* stats, double* cost, double* loop_chi2, hipStream_t s) {
  const int grid = graphs < kPgResident ? graphs : kPgResident;
  hipLaunchKernelGGL(k_pg_solve, dim3(grid), dim3(kPgThreads), 0, s, n_nodes, pose0, odom_z, odom_sigma, loop_ij, loop_z, loop_sigma, loop_k2,
                     loop_enable, N, L, graphs, k, static_cast<char*>(ws), pg_workspace_bytes(N, L), pose, stats, cost, loop_chi2);
}
void launch_pg_odometry(const double* pose, int N, int graphs, double* odom_z, hipStream_t s) {
  const long long total = (long long)graphs * (N - 1);
  hipLaunchKernelGGL(k_pg_odometry, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, pose, N, total, odom_z);
}
void launch_pg_loops(const int32_t* from, const int32_t* to, const double* pose, const int32_t* stats, int pairs, int min_inliers,
                     double noise_base, int32_t* loop_ij, double* loop_z, double* loop_sigma, double* loop_k2, uint8_t* loop_enable,
                     hipStream_t s) {
  hipLaunchKernelGGL(k_pg_loops, dim3((pairs + 255) / 256), dim3(256), 0, s, from, to, pose, stats, pairs, min_inliers, noise_base, loop_ij,
                     loop_z, loop_sigma, loop_k2, loop_enable);
}

}  // namespace sship
