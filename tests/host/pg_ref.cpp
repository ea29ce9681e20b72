// TEST INFRASTRUCTURE ONLY. An independent CPU restatement of the pose-graph optimisation of include/mloam_hip.h section (f14), built with plain g++ and
// -ffp-contract=off by tests/pg_cases.py and called through ctypes. It shares no code with m-loam_amd/csrc/pg_host.hpp or the kernels:
//   - the factor (what RelativeRTError computes, mloam_loop/include/mloam_loop/pose_graph.h:299-337, in this project's own words over pose arrays) is evaluated
//     over a forward-mode dual type with 14 derivatives (the seven stored values of each of the two poses), as ceres::AutoDiffCostFunction does, and the ambient 6 x 4 blocks are multiplied by the 4 x 3 Jacobian of
//     ceres::QuaternionParameterization;
//   - HuberLoss through Ceres's Corrector (rho'' <= 0: residual and Jacobian scaled by sqrt(rho'));
//   - the dense H = J^T J, g = J^T r feed ceres_like_solve_dyn of oracle/lm.hpp, whose linear solve is oracle/linalg.hpp's dense cholesky_d. lm.hpp reaches it
//     through chol_solve_d, whose work arrays are fixed at 32 unknowns; this file routes that one call to the same factorisation and the same two substitutions
//     over heap arrays (the macro below), leaving oracle/ as it is;
//   - the write-back and the drift propagation (mloam_loop/src/pose_graph.cpp:615-641; KeyFrame::updatePose; Pose(q, t), inverse, operator*), with Eigen's
//     quaternion product, inverse, normalize and q * v written out in Eigen's own term order.
// Ceres and Eigen are restated from memory of Ceres 1.12 / Eigen 3.3 (neither is available to this project).
// Poses are [t, q(xyzw)]; local blocks are [rotation 3, translation 3] (Ceres orders q before t: pose_graph.cpp:546-547). x of the solve holds the free
// keyframes' poses (the constant first block is not part of the reduced problem).
#include "linalg.hpp"
#include <vector>
namespace orc {
// pgr_optimize's handle on the solver's linear solves: call k (= iteration k + 1) is refused when bit k of fail_mask is set -- what a non-positive pivot would
// do --, and the first diagonal entry of every system handed in is kept (the radius it was formed with is read back from it)
struct PgrSolveHook { unsigned fail_mask = 0u; int calls = 0, refused = 0; double lhs00 = 0.0; };
static PgrSolveHook pgr_hook;
static inline bool pgr_chol_solve_heap(const double *A, const double *b, int n, double *x)
{
    const int call = pgr_hook.calls++;
    if (n > 0) pgr_hook.lhs00 = A[0];
    if (call < 32 && ((pgr_hook.fail_mask >> call) & 1u)) { ++pgr_hook.refused; return false; }
    std::vector<double> L(size_t(n) * size_t(n)), y(size_t(n) + 1);
    if (!cholesky_d(A, n, L.data())) return false;
    for (int i = 0; i < n; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s -= L[size_t(i) * n + k] * y[k];
        y[i] = s / L[size_t(i) * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < n; ++k) s -= L[size_t(k) * n + i] * x[k];
        x[i] = s / L[size_t(i) * n + i];
    }
    return true;
}
}  // namespace orc
#define chol_solve_d pgr_chol_solve_heap
#include "lm.hpp"
#undef chol_solve_d
#include <cmath>
#include <cstdint>
#include <cstring>

namespace {

constexpr int ND = 14;
struct Dual {
    double v;
    double d[ND];
    Dual() : v(0.0) { for (int i = 0; i < ND; ++i) d[i] = 0.0; }
    Dual(double c) : v(c) { for (int i = 0; i < ND; ++i) d[i] = 0.0; }   // NOLINT: constants convert, as with ceres::Jet
};
Dual operator+(const Dual &a, const Dual &b) { Dual r; r.v = a.v + b.v; for (int i = 0; i < ND; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
Dual operator-(const Dual &a, const Dual &b) { Dual r; r.v = a.v - b.v; for (int i = 0; i < ND; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
Dual operator-(const Dual &a) { Dual r; r.v = -a.v; for (int i = 0; i < ND; ++i) r.d[i] = -a.d[i]; return r; }
Dual operator*(const Dual &a, const Dual &b) { Dual r; r.v = a.v * b.v; for (int i = 0; i < ND; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i]; return r; }
Dual operator/(const Dual &a, const Dual &b)
{
    Dual r;
    r.v = a.v / b.v;
    for (int i = 0; i < ND; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) / b.v;
    return r;
}
Dual sqrt(const Dual &a) { Dual r; r.v = std::sqrt(a.v); for (int i = 0; i < ND; ++i) r.d[i] = a.d[i] / (2.0 * r.v); return r; }
double sqrt(double a) { return std::sqrt(a); }

// ceres::QuaternionProduct, (w, x, y, z)
template <typename T> void quat_product(const T z[4], const T w[4], T zw[4])
{
    zw[0] = z[0] * w[0] - z[1] * w[1] - z[2] * w[2] - z[3] * w[3];
    zw[1] = z[0] * w[1] + z[1] * w[0] + z[2] * w[3] - z[3] * w[2];
    zw[2] = z[0] * w[2] - z[1] * w[3] + z[2] * w[0] + z[3] * w[1];
    zw[3] = z[0] * w[3] + z[1] * w[2] - z[2] * w[1] + z[3] * w[0];
}
// ceres::QuaternionRotatePoint: normalise, then UnitQuaternionRotatePoint
template <typename T> void quat_rotate_point(const T q[4], const T pt[3], T result[3])
{
    const T scale = T(1.0) / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const T u[4] = {scale * q[0], scale * q[1], scale * q[2], scale * q[3]};
    const T t2 = u[0] * u[1], t3 = u[0] * u[2], t4 = u[0] * u[3], t5 = -u[1] * u[1], t6 = u[1] * u[2], t7 = u[1] * u[3], t8 = -u[2] * u[2], t9 = u[2] * u[3],
            t1 = -u[3] * u[3];
    result[0] = T(2.0) * ((t8 + t1) * pt[0] + (t6 - t4) * pt[1] + (t3 + t7) * pt[2]) + pt[0];
    result[1] = T(2.0) * ((t4 + t6) * pt[0] + (t5 + t1) * pt[1] + (t9 - t2) * pt[2]) + pt[1];
    result[2] = T(2.0) * ((t7 - t3) * pt[0] + (t2 + t9) * pt[1] + (t5 + t8) * pt[2]) + pt[2];
}
template <typename T> void quat_conjugate(const T q[4], T c[4]) { c[0] = q[0]; c[1] = -q[1]; c[2] = -q[2]; c[3] = -q[3]; }   // what pose_graph.h:121-127 computes

// The relative-pose residual of one edge, written over the project's pose arrays [t, q(xyzw)] and templated on the scalar (double, or Dual for the derivatives).
// It replaces the reference's factor (mloam_loop/include/mloam_loop/pose_graph.h:299-337): the translation of keyframe b seen from keyframe a, less the measured
// one, over t_var; then twice the vector part of measured^-1 (x) (a^-1 (x) b), over q_var. "Inverse" is the conjugate, as there; the point rotation normalises.
template <typename S> void relative_pose_residual(const S a[7], const S b[7], const double measured[7], double t_var, double q_var, S out[6])
{
    const S qa[4] = {a[6], a[3], a[4], a[5]}, qb[4] = {b[6], b[3], b[4], b[5]};
    const S qm[4] = {S(measured[6]), S(measured[3]), S(measured[4]), S(measured[5])};
    S qa_c[4], qm_c[4];
    quat_conjugate(qa, qa_c);
    quat_conjugate(qm, qm_c);
    const S baseline[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    S seen[3];
    quat_rotate_point(qa_c, baseline, seen);
    for (int k = 0; k < 3; ++k) out[k] = (seen[k] - S(measured[k])) / S(t_var);
    S a_to_b[4], mismatch[4];
    quat_product(qa_c, qb, a_to_b);
    quat_product(qm_c, a_to_b, mismatch);
    for (int k = 0; k < 3; ++k) out[3 + k] = S(2.0) * mismatch[1 + k] / S(q_var);
}

// QuaternionParameterization::ComputeJacobian at x = (w, x, y, z): 4 x 3 row-major
void param_jacobian(const double x[4], double J[12])
{
    J[0] = -x[1]; J[1] = -x[2]; J[2] = -x[3];
    J[3] = x[0];  J[4] = x[3];  J[5] = -x[2];
    J[6] = -x[3]; J[7] = x[0];  J[8] = x[1];
    J[9] = x[2];  J[10] = -x[1]; J[11] = x[0];
}
// QuaternionParameterization::Plus
void param_plus(const double x[4], const double delta[3], double out[4])
{
    const double norm_delta = std::sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]);
    if (norm_delta > 0.0) {
        const double sin_delta_by_delta = std::sin(norm_delta) / norm_delta;
        const double q_delta[4] = {std::cos(norm_delta), sin_delta_by_delta * delta[0], sin_delta_by_delta * delta[1], sin_delta_by_delta * delta[2]};
        quat_product(q_delta, x, out);
    } else {
        for (int i = 0; i < 4; ++i) out[i] = x[i];
    }
}

void wxyz(const double p[7], double q[4]) { q[0] = p[6]; q[1] = p[3]; q[2] = p[4]; q[3] = p[5]; }

// the uncorrected residual and local Jacobians of one edge: derivative slot 7 e + c belongs to component c of pose e (0: i, 1: j), in the pose's own layout
void edge_eval(const double pi[7], const double pj[7], const double meas[7], double t_var, double q_var, double r[6], double Ji[36], double Jj[36])
{
    Dual di[7], dj[7], res[6];
    for (int c = 0; c < 7; ++c) { di[c] = Dual(pi[c]); di[c].d[c] = 1.0; dj[c] = Dual(pj[c]); dj[c].d[7 + c] = 1.0; }
    relative_pose_residual(di, dj, meas, t_var, q_var, res);
    double qi[4], qj[4], Pi[12], Pj[12];
    wxyz(pi, qi); wxyz(pj, qj);
    param_jacobian(qi, Pi); param_jacobian(qj, Pj);
    // where (w, x, y, z) sit in a pose: 6, 3, 4, 5
    const int slot[4] = {6, 3, 4, 5};
    for (int a = 0; a < 6; ++a) {
        r[a] = res[a].v;
        for (int c = 0; c < 3; ++c) {
            double si = 0.0, sj = 0.0;
            for (int k = 0; k < 4; ++k) { si += res[a].d[slot[k]] * Pi[k * 3 + c]; sj += res[a].d[7 + slot[k]] * Pj[k * 3 + c]; }
            Ji[a * 6 + c] = si; Jj[a * 6 + c] = sj;
            Ji[a * 6 + 3 + c] = res[a].d[c]; Jj[a * 6 + 3 + c] = res[a].d[7 + c];
        }
    }
}

// Eigen: a * b, a.inverse(), q * v, normalize -- in Eigen's term order
void eig_qmul(const double a[4], const double b[4], double o[4])
{
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
    o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}
void eig_qinv(const double q[4], double o[4])
{
    const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (n2 > 0.0) { o[0] = q[0] / n2; o[1] = -q[1] / n2; o[2] = -q[2] / n2; o[3] = -q[3] / n2; }
    else o[0] = o[1] = o[2] = o[3] = 0.0;
}
void eig_qrot(const double q[4], const double v[3], double o[3])
{
    double uv[3] = {q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]};
    for (int c = 0; c < 3; ++c) uv[c] += uv[c];
    const double cx[3] = {q[2] * uv[2] - q[3] * uv[1], q[3] * uv[0] - q[1] * uv[2], q[1] * uv[1] - q[2] * uv[0]};
    for (int c = 0; c < 3; ++c) o[c] = v[c] + q[0] * uv[c] + cx[c];
}
struct PoseR {
    double q[4], t[3];
    PoseR() : q{1.0, 0.0, 0.0, 0.0}, t{0.0, 0.0, 0.0} {}
    PoseR(const double qq[4], const double tt[3])          // Pose(q, t): q_.normalize()
    {
        const double n = std::sqrt(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3]);
        for (int c = 0; c < 4; ++c) q[c] = n != 0.0 ? qq[c] / n : qq[c];
        for (int c = 0; c < 3; ++c) t[c] = tt[c];
    }
    explicit PoseR(const double p[7]) { wxyz(p, q); t[0] = p[0]; t[1] = p[1]; t[2] = p[2]; }    // stored as it is
    void store(double p[7]) const { p[0] = t[0]; p[1] = t[1]; p[2] = t[2]; p[3] = q[1]; p[4] = q[2]; p[5] = q[3]; p[6] = q[0]; }
    PoseR inverse() const
    {
        double qi[4], ti[3];
        eig_qinv(q, qi);
        eig_qrot(qi, t, ti);
        for (int c = 0; c < 3; ++c) ti[c] = -ti[c];
        return PoseR(qi, ti);
    }
    PoseR operator*(const PoseR &o) const
    {
        double qq[4], tt[3];
        eig_qmul(q, o.q, qq);
        eig_qrot(q, o.t, tt);
        for (int c = 0; c < 3; ++c) tt[c] += t[c];
        return PoseR(qq, tt);
    }
};

struct Edge { int i, j, loop; double meas[7]; };

struct Problem {
    int M = 0, first = 0;
    double t_var = 0.1, q_var = 0.01, huber = 1.0;
    std::vector<Edge> edges;
    std::vector<double> x0;          // M x 7
};

// the problem of cpp:530-601 over keyframes first..cur
Problem build(const double *poses, const int32_t *loop_index, const double *loop_rel, int first, int cur, double t_var, double q_var, double huber)
{
    Problem P;
    P.M = cur - first + 1; P.first = first; P.t_var = t_var; P.q_var = q_var; P.huber = huber;
    P.x0.assign(poses + size_t(first) * 7, poses + size_t(cur + 1) * 7);
    for (int i = 0; i < P.M; ++i) {
        for (int j = 1; j < 5; ++j)
            if (i - j >= 0) {
                const PoseR a(&P.x0[size_t(i - j) * 7]), b(&P.x0[size_t(i) * 7]);
                Edge e;
                e.i = i - j; e.j = i; e.loop = 0;
                double qi[4], rq[4], rt[3];
                const double dt[3] = {b.t[0] - a.t[0], b.t[1] - a.t[1], b.t[2] - a.t[2]};
                eig_qinv(a.q, qi);
                eig_qrot(qi, dt, rt);
                eig_qmul(qi, b.q, rq);
                e.meas[0] = rt[0]; e.meas[1] = rt[1]; e.meas[2] = rt[2]; e.meas[3] = rq[1]; e.meas[4] = rq[2]; e.meas[5] = rq[3]; e.meas[6] = rq[0];
                P.edges.push_back(e);
            }
        const int li = loop_index[first + i];
        if (li >= 0) {
            Edge e;
            e.i = li - first; e.j = i; e.loop = 1;
            std::memcpy(e.meas, loop_rel + size_t(first + i) * 7, sizeof(e.meas));
            P.edges.push_back(e);
        }
    }
    return P;
}

// pose k of the problem at x (the free blocks' poses; block 0 from x0)
const double *pose_at(const Problem &P, const double *x, int k) { return k == 0 ? P.x0.data() : x + size_t(k - 1) * 7; }

// corrected residual / Jacobians of edge e at x; returns rho / 2
double edge_corrected(const Problem &P, const Edge &e, const double *x, double r[6], double Ji[36], double Jj[36])
{
    edge_eval(pose_at(P, x, e.i), pose_at(P, x, e.j), e.meas, P.t_var, P.q_var, r, Ji, Jj);
    double s = 0.0;
    for (int c = 0; c < 6; ++c) s += r[c] * r[c];
    if (!e.loop) return 0.5 * s;
    double rho0 = s, rho1 = 1.0;
    const double b = P.huber * P.huber;
    if (s > b) { const double rr = std::sqrt(s); rho0 = 2.0 * P.huber * rr - b; rho1 = P.huber / rr; }
    const double sc = std::sqrt(rho1);
    for (int c = 0; c < 6; ++c) r[c] *= sc;
    for (int c = 0; c < 36; ++c) { Ji[c] *= sc; Jj[c] *= sc; }
    return 0.5 * rho0;
}

void evaluate(const Problem &P, const double *x, orc::NormalEqDyn &ne)
{
    const size_t n = size_t(6 * (P.M - 1));
    ne.H.assign(n * n, 0.0); ne.g.assign(n, 0.0); ne.cost = 0.0; ne.count = int(P.edges.size());
    for (const Edge &e : P.edges) {
        double r[6], J[2][36];
        ne.cost += edge_corrected(P, e, x, r, J[0], J[1]);
        const int blk[2] = {e.i - 1, e.j - 1};
        for (int u = 0; u < 2; ++u) {
            if (blk[u] < 0) continue;
            for (int a = 0; a < 6; ++a) {
                double w = 0.0;
                for (int q = 0; q < 6; ++q) w += J[u][q * 6 + a] * r[q];
                ne.g[size_t(blk[u]) * 6 + a] += w;
            }
            for (int v = 0; v < 2; ++v) {
                if (blk[v] < 0) continue;
                for (int a = 0; a < 6; ++a)
                    for (int c = 0; c < 6; ++c) {
                        double acc = 0.0;
                        for (int q = 0; q < 6; ++q) acc += J[u][q * 6 + a] * J[v][q * 6 + c];
                        ne.H[(size_t(blk[u]) * 6 + a) * n + size_t(blk[v]) * 6 + c] += acc;
                    }
            }
        }
    }
}

void plus_all(int nb, const double *x, const double *delta, double *out)
{
    for (int b = 0; b < nb; ++b) {
        const double *p = x + size_t(b) * 7, *d = delta + size_t(b) * 6;
        double *o = out + size_t(b) * 7;
        double q[4], qo[4];
        wxyz(p, q);
        param_plus(q, d, qo);
        o[0] = p[0] + d[3]; o[1] = p[1] + d[4]; o[2] = p[2] + d[5];
        o[3] = qo[1]; o[4] = qo[2]; o[5] = qo[3]; o[6] = qo[0];
    }
}

}  // namespace

extern "C" {

struct pgr_opts { int max_num_iterations, pad; double t_var, q_var, huber_delta; };
struct pgr_result {
    int num_iterations, num_successful_steps, termination, n_keyframes, n_loops, n_decisions;
    int n_rejected, n_refused;    // candidates the policy turned down (relative decrease <= 1e-3, model change <= 0); linear solves refused by fail_mask
    double initial_cost, final_cost, drift[7];
    double min_margin;            // the smallest relative distance of a decision quantity of the run from its threshold
    double margin_relative_decrease, margin_function, margin_parameter, margin_gradient, margin_model;
    double solve_radius;          // the radius of the last linear system: clamp(A00) / (lhs00 - A00) of its first diagonal entry (good to ~1e-11 relative)
};

void pgr_edge(const double *pi, const double *pj, const double *meas, double t_var, double q_var, double *r, double *Ji, double *Jj)
{
    edge_eval(pi, pj, meas, t_var, q_var, r, Ji, Jj);
}

void pgr_plus(const double *x, const double *delta, double *out) { plus_all(1, x, delta, out); }

void pgr_pose_mul(const double *a, const double *b, double *out) { (PoseR(a) * PoseR(b)).store(out); }
void pgr_pose_inverse(const double *a, double *out) { PoseR(a).inverse().store(out); }

// the edges in the reference's order, corrected; dense H, g (may be null)
int pgr_linearize(const double *poses, const int32_t *loop_index, const double *loop_rel, int first, int cur, const pgr_opts *o, int32_t *ij, double *r, double *Ji,
                  double *Jj, double *cost, double *H, double *g)
{
    const Problem P = build(poses, loop_index, loop_rel, first, cur, o->t_var, o->q_var, o->huber_delta);
    const double *x = P.x0.data() + 7;
    int ne = 0;
    double c = 0.0;
    for (const Edge &e : P.edges) {
        ij[2 * ne] = e.i; ij[2 * ne + 1] = e.j;
        c += edge_corrected(P, e, x, r + size_t(ne) * 6, Ji + size_t(ne) * 36, Jj + size_t(ne) * 36);
        ++ne;
    }
    *cost = c;
    if (H && g) {
        orc::NormalEqDyn d;
        evaluate(P, x, d);
        std::memcpy(H, d.H.data(), sizeof(double) * d.H.size());
        std::memcpy(g, d.g.data(), sizeof(double) * d.g.size());
    }
    return ne;
}

// one linear solve as ceres_like_solve_dyn's first iteration forms it, from given normal equations: returns 1 when the factorisation succeeded
int pgr_dense_step(const double *H, const double *g, int n, double radius, double *step, double *delta)
{
    const size_t N = size_t(n);
    if (N == 0) return 1;
    std::vector<double> S(N), A(N * N), gs(N), y(N);
    for (size_t i = 0; i < N; ++i) S[i] = 1.0 / (1.0 + std::sqrt(H[i * N + i]));
    for (size_t rr = 0; rr < N; ++rr) {
        gs[rr] = S[rr] * g[rr];
        for (size_t c = 0; c < N; ++c) A[rr * N + c] = S[rr] * H[rr * N + c] * S[c];
    }
    for (size_t i = 0; i < N; ++i) A[i * N + i] += std::min(std::max(A[i * N + i], 1e-6), 1e32) / radius;
    if (!orc::pgr_chol_solve_heap(A.data(), gs.data(), int(N), y.data())) return 0;
    for (size_t i = 0; i < N; ++i) { step[i] = -y[i]; delta[i] = step[i] * S[i]; }
    return 1;
}

// ... at the graph's poses
int pgr_solve_step(const double *poses, const int32_t *loop_index, const double *loop_rel, int first, int cur, const pgr_opts *o, double radius, double *step, double *delta)
{
    const Problem P = build(poses, loop_index, loop_rel, first, cur, o->t_var, o->q_var, o->huber_delta);
    if (P.M < 2) return 1;
    orc::NormalEqDyn ne;
    evaluate(P, P.x0.data() + 7, ne);
    return pgr_dense_step(ne.H.data(), ne.g.data(), 6 * (P.M - 1), radius, step, delta);
}

// one pass of optimizePoseGraph's body: poses / last (count x 7) are updated in place
void pgr_optimize(double *poses, double *last, const int32_t *loop_index, const double *loop_rel, int count, int first, int cur, const pgr_opts *o, unsigned fail_mask,
                  pgr_result *res)
{
    orc::pgr_hook = orc::PgrSolveHook();
    orc::pgr_hook.fail_mask = fail_mask;
    const Problem P = build(poses, loop_index, loop_rel, first, cur, o->t_var, o->q_var, o->huber_delta);
    const int nb = P.M - 1;
    const size_t N = size_t(6 * nb), NX = size_t(7 * nb);
    std::vector<double> x(P.x0.begin() + 7, P.x0.end());
    x.resize(NX + 1);
    // the decision quantities, reconstructed from what the solver hands to its two callbacks
    orc::NormalEqDyn cur_ne, last_ne, solve_ne;
    double first_H00 = 0.0;
    std::vector<double> c_x, c_delta, c_out;
    bool have_cand = false;
    int n_eval = 0;
    const double INF = 1e300;
    double m_rd = INF, m_fn = INF, m_par = INF, m_grad = INF, m_model = INF;
    int n_dec = 0, n_rej = 0;
    const auto rel = [](double q, double thr) { return std::fabs(q - thr) / std::max(std::fabs(thr), 1e-300); };
    const auto ev = [&](const double *at, orc::NormalEqDyn &d) {
        evaluate(P, at, d);
        ++n_eval;
        if (n_eval == 1 && N > 0) { first_H00 = d.H[0]; solve_ne = d; }
        if (n_eval > 1 && have_cand) {
            double sg = 0.0, sHs = 0.0;
            for (size_t rr = 0; rr < N; ++rr) {
                sg += c_delta[rr] * cur_ne.g[rr];
                double t = 0.0;
                for (size_t c = 0; c < N; ++c) t += cur_ne.H[rr * N + c] * c_delta[c];
                sHs += c_delta[rr] * t;
            }
            const double model = -(sg + 0.5 * sHs);
            m_model = std::min(m_model, std::fabs(model) / std::max(std::fabs(sg) + 0.5 * std::fabs(sHs), 1e-300)); ++n_dec;
            double sn = 0.0, xn = 0.0;
            for (size_t i = 0; i < NX; ++i) { sn += (c_x[i] - c_out[i]) * (c_x[i] - c_out[i]); xn += c_x[i] * c_x[i]; }
            sn = std::sqrt(sn); xn = std::sqrt(xn);
            const double pthr = 1e-8 * (xn + 1e-8);
            m_par = std::min(m_par, rel(sn, pthr)); ++n_dec;
            if (model > 0.0 && sn > pthr) {
                const double cc = cur_ne.cost - d.cost, fthr = 1e-6 * cur_ne.cost;
                m_fn = std::min(m_fn, rel(std::fabs(cc), fthr)); ++n_dec;
                if (std::fabs(cc) > fthr) { m_rd = std::min(m_rd, rel(cc / model, 1e-3)); ++n_dec; n_rej += !(cc / model > 1e-3); }
            } else if (!(model > 0.0)) ++n_rej;
            have_cand = false;
        }
        last_ne = d;
    };
    const auto pl = [&](const double *at, const double *dl, double *out) {
        plus_all(nb, at, dl, out);
        bool is_gradient = true;
        for (size_t i = 0; i < N && is_gradient; ++i) is_gradient = dl[i] == -last_ne.g[i];
        if (is_gradient) {
            cur_ne = last_ne;                       // the evaluation the solver now holds as its current point
            solve_ne = cur_ne;                      // ... and forms its next system at
            double gm = 0.0;
            for (size_t i = 0; i < NX; ++i) gm = std::max(gm, std::fabs(at[i] - out[i]));
            m_grad = std::min(m_grad, rel(gm, 1e-10)); ++n_dec;
        } else {
            c_x.assign(at, at + NX); c_delta.assign(dl, dl + N); c_out.assign(out, out + NX);
            have_cand = true;
        }
    };
    orc::SolveSummary sum;
    orc::ceres_like_solve_dyn(ev, pl, x.data(), int(N), int(NX), o->max_num_iterations, sum);
    std::memset(res, 0, sizeof(*res));
    res->n_refused = orc::pgr_hook.refused;
    res->solve_radius = 1e4;
    if (orc::pgr_hook.calls > 0 && N > 0) {
        // the solver's current point when it formed its last system is cur_ne unless that system's step was then accepted (the last call of a run never is
        // followed by another system, so an accepted last step leaves cur_ne one evaluation ahead: keep the point the system was formed at)
        const orc::NormalEqDyn &at = solve_ne;
        const double S0 = 1.0 / (1.0 + std::sqrt(first_H00)), A00 = S0 * at.H[0] * S0;
        res->solve_radius = std::min(std::max(A00, 1e-6), 1e32) / (orc::pgr_hook.lhs00 - A00);
    }
    orc::pgr_hook = orc::PgrSolveHook();
    res->num_iterations = sum.num_iterations; res->num_successful_steps = sum.num_successful_steps; res->termination = sum.termination;
    res->n_keyframes = P.M; res->n_decisions = n_dec; res->n_rejected = n_rej;
    for (const Edge &e : P.edges) res->n_loops += e.loop;
    res->initial_cost = sum.initial_cost; res->final_cost = sum.final_cost;
    res->margin_relative_decrease = m_rd; res->margin_function = m_fn; res->margin_parameter = m_par; res->margin_gradient = m_grad; res->margin_model = m_model;
    res->min_margin = std::min(std::min(std::min(m_rd, m_fn), std::min(m_par, m_grad)), m_model);
    // cpp:615-627
    for (int k = 0; k < P.M; ++k) {
        const double *p = pose_at(P, x.data(), k);
        double q[4];
        wxyz(p, q);
        const PoseR np(q, p);
        double *dst = poses + size_t(first + k) * 7;
        std::memcpy(last + size_t(first + k) * 7, dst, sizeof(double) * 7);
        np.store(dst);
    }
    // cpp:630-641
    const PoseR cur_pose(poses + size_t(cur) * 7), last_pose(last + size_t(cur) * 7);
    const PoseR drift = PoseR(cur_pose) * last_pose.inverse();
    drift.store(res->drift);
    for (int k = cur + 1; k < count; ++k) {
        double *dst = poses + size_t(k) * 7;
        const PoseR up = PoseR(drift) * PoseR(dst);
        std::memcpy(last + size_t(k) * 7, dst, sizeof(double) * 7);
        up.store(dst);
    }
}

}  // extern "C"
