// The vocabulary of the instruction tape (include/optas_hip.h: oh_tape_desc), stated once: the opcodes' names, how many operands each reads, its
// value, its first-order adjoint rule, which registers the cost and the rows depend on.  Every device evaluator is written against this file: the
// interpreter and oh_tape_probe (oh_tape.hip) and the QP assembly (oh_qp.hip) apply the rules; oh_tape_hvp and the wavefront evaluator (oh_tape_wave.hip) take the names and the host side.
//
// A RULE CHANGED HERE MUST ALSO BE CHANGED where rules are stated again:
//   * generate() in oh_tape.hip, deliberately: it writes the rules as text for hiprtc (its two emit tables), and that text is what tests read, what
//     keys the disk cache and what sets the compile time;
//   * k_tape_hvp (oh_tape.hip), which has every primal line beside its second-order lines: through this header its bits were the same and the
//     planner's dense Hessian 0.5 % slower;
//   * InterpEval::hess_vec (oh_tape.hip), the tangent and second-order lines of k_tape_hvp once more without the primal accumulations beside them:
//     it runs on the adjoints a finished reverse sweep left and must not repeat them;
//   * WaveEval::sweep (oh_tape_wave.hip), the wavefront evaluator's ONE statement: the rare-path switches of its forward and reverse pass hold the value,
//     the adjoint rule and, under `if constexpr (TAN)`, the tangent and second-order lines of the opcodes the straight-line path does not cover; every
//     wavefront kernel (evaluation, products with given weights, products of the merit, both solvers) runs that one body.  It stays outside tape_value /
//     tape_adjoint because it works on operands the pass has loaded already -- through this header the forward switch was 3 % slower on the planner --
//     and because the wavefront's reverse sweep has no accumulation to differentiate: an instruction leaves its contribution to each operand as a VALUE
//     in its own slots (ca, cb) and the consumers' slots are gathered later, so each rule is the pair (contribution, its directional derivative) of
//     one operand, and an accessor that stored them through a pointer put them in scratch memory;
//   * ADD, SUB and MUL in the two sweeps of the QP assembly (oh_qp.hip), 0.5 - 2 % faster as cases of their own.
// The measured reasons are written at each.  All of them use the names below.
// tests/test_gpu_tape_evaluators.py and tests/test_gpu_tape_hvp.py hold all of them together bit for bit, tests/test_gpu_tape_hvp_wave.py k_tape_wave_hvp to the 60-digit reference, tests/test_gpu_tape_newton.py hess_vec and tests/test_gpu_tape_newton_wave.py the merit's products on WaveEval::sweep to the 60-digit reference; tests/test_gpu_tape_wave_bits.py pins the sweep's bits.  Independent restatements: optas_amd/tape.py, oracle/tape_ref.py, oracle/tape_mp.py.
//
// A rule takes its operands through a small accessor R of the caller -- values: cst(), x(), p() (what CONST, X and P load, from wherever the caller
// keeps constants, the point and the parameters), a(), b(), self() (the instruction's own value); contributions: add_a(v), add_b(v), sub_a(v),
// sub_b(v), add_x(v) (to the gradient entry of X's variable) -- and touches only what it names: ADD's adjoint loads no value, a unary opcode never reads b (b[i] of a unary instruction is not validated), SQRT and
// EXP read their own result.  The interpreter's accessor is a load from / a read-modify-write of its register file in memory (one dependent round
// trip each: what that evaluator is bound by); the QP assembly's serves tape_value alone.
// What callers rely on: a rule that subtracts says so (sub_a, sub_b) and never adds a negation -- the compiler leaves a unary minus open to
// contraction whatever the pragma says, and x + (-(w s)) came out as one fused operation, an ulp from x - w s; FMIN / FMAX / IFZ select an operand,
// they never multiply the other by 0.  One IEEE operation or one libm call per step, in the
// order written, as the numpy restatement and casadi's SX machine compute them: contraction is off in every body (the pragma of a caller does not
// reach into an inlined function, and atan2's va * va + vb * vb would fuse).
#ifndef OH_TAPE_OPS_H
#define OH_TAPE_OPS_H

#include <vector>

// the numbering of optas_amd/tape.py
enum TapeOp : int {
  OP_CONST = 0, OP_X, OP_P, OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_NEG, OP_SIN, OP_COS, OP_ATAN2, OP_SQRT, OP_SQR,  // 0 .. 12
  OP_ASIN, OP_FABS, OP_FMIN, OP_FMAX, OP_LT, OP_LE, OP_EQ, OP_NE, OP_NOT, OP_AND, OP_OR, OP_IFZ,                // 13 .. 24: what Quaternion.getrpy and optas.clip emit
  OP_EXP, OP_LOG,  // 25, 26: with them the walker expresses pow, tanh, sinh, cosh, acos, atan, the inverse hyperbolics (casadi_tape.py)
  OP_COUNT
};
// Bit 5 of an opcode in the interpreter's device copy: neither the cost nor a row depends on the instruction (oh_create_tape sets it from tape_live).
// Its reverse sweep passes such an instruction by, as the generated code and the wavefront schedule leave it out: the adjoint is 0, but 0 times a
// non-finite partial derivative (a dead x / 0) is not.
constexpr int OP_DEAD = 32, OP_MASK = OP_DEAD - 1;

// operands an instruction reads: 0 (CONST, X, P), 1 or 2
__host__ __device__ inline int tape_op_arity(const int o) {
  if (o <= OP_P) return 0;
  return ((o >= OP_ADD && o <= OP_DIV) || o == OP_ATAN2 || (o >= OP_FMIN && o <= OP_NE) || (o >= OP_AND && o <= OP_IFZ)) ? 2 : 1;
}
// whether the register carries an adjoint (CONST and P do not: nothing is differentiated with respect to them)
__host__ __device__ inline bool tape_op_has_adjoint(const int o) { return o != OP_CONST && o != OP_P; }

// live[i] != 0: the cost or a row depends on register i (what the reverse sweep reaches, what generated code and the wavefront schedule contain)
inline std::vector<char> tape_live(const int len, const int* op, const int* a, const int* b, const int* rows, const int n_rows, const int out_cost) {
  std::vector<char> live(len, 0);
  live[out_cost] = 1;
  for (int i = 0; i < n_rows; ++i) live[rows[i]] = 1;
  for (int i = len - 1; i >= 0; --i) {
    if (!live[i]) continue;
    const int n = tape_op_arity(op[i]);
    if (n >= 1) live[a[i]] = 1;
    if (n == 2) live[b[i]] = 1;
  }
  return live;
}

// Value of instruction o.  (One flat switch over all of them on purpose: with CONST, X and P in a switch of the caller around this one, every case
// left here begins with the load of a, the compiler moves that load in front of the switch and the load of b then waits for it -- two dependent
// round trips a binary instruction where there was one, +19 % on the interpreter's solve of the 7-joint IK tape at 65 536 instances.)
template <class R>
__device__ __attribute__((always_inline)) inline double tape_value(const int o, const R& r) {
#pragma clang fp contract(off)
  switch (o) {
    case OP_CONST: return r.cst();
    case OP_X: return r.x();
    case OP_P: return r.p();
    case OP_ADD: return r.a() + r.b();
    case OP_SUB: return r.a() - r.b();
    case OP_MUL: return r.a() * r.b();
    case OP_DIV: return r.a() / r.b();
    case OP_NEG: return -r.a();
    case OP_SIN: return sin(r.a());
    case OP_COS: return cos(r.a());
    case OP_ATAN2: return atan2(r.a(), r.b());
    case OP_SQRT: return sqrt(r.a());
    case OP_SQR: { const double va = r.a(); return va * va; }
    case OP_ASIN: return asin(r.a());
    case OP_FABS: return fabs(r.a());
    case OP_FMIN: return fmin(r.a(), r.b());
    case OP_FMAX: return fmax(r.a(), r.b());
    case OP_LT: return r.a() < r.b() ? 1.0 : 0.0;
    case OP_LE: return r.a() <= r.b() ? 1.0 : 0.0;
    case OP_EQ: return r.a() == r.b() ? 1.0 : 0.0;
    case OP_NE: return r.a() != r.b() ? 1.0 : 0.0;
    case OP_NOT: return r.a() == 0.0 ? 1.0 : 0.0;
    case OP_AND: return (r.a() != 0.0 && r.b() != 0.0) ? 1.0 : 0.0;
    case OP_OR: return (r.a() != 0.0 || r.b() != 0.0) ? 1.0 : 0.0;
    case OP_IFZ: return r.a() != 0.0 ? r.b() : 0.0;  // casadi's if_else_zero
    case OP_EXP: return exp(r.a());
    default: return log(r.a());  // OP_LOG
  }
}

// Reverse rule of instruction o whose adjoint is w: r.add_a(w d value / d a), r.add_b(w d value / d b) (sub_a, sub_b: the same, subtracted); X hands its
// adjoint to the gradient.  Nothing for CONST and P, nothing for LT .. OR (piecewise constant).  Derivative conventions of ASIN .. FMAX and IFZ are casadi's (casadi/core/calculus.hpp).
template <class R>
__device__ __attribute__((always_inline)) inline void tape_adjoint(const int o, const double w, R& r) {
#pragma clang fp contract(off)
  switch (o) {
    case OP_X: r.add_x(w); break;
    case OP_ADD: r.add_a(w); r.add_b(w); break;
    case OP_SUB: r.add_a(w); r.sub_b(w); break;
    case OP_MUL: { const double va = r.a(), vb = r.b(); r.add_a(w * vb); r.add_b(w * va); } break;  // (MUL a a: two accumulations into the one register)
    case OP_DIV: { const double va = r.a(), vb = r.b(); r.add_a(w / vb); r.sub_b(w * va / (vb * vb)); } break;
    case OP_NEG: r.sub_a(w); break;
    case OP_SIN: r.add_a(w * cos(r.a())); break;
    case OP_COS: r.sub_a(w * sin(r.a())); break;
    case OP_ATAN2: { const double va = r.a(), vb = r.b(), d = va * va + vb * vb; r.add_a(w * vb / d); r.sub_b(w * va / d); } break;
    case OP_SQRT: r.add_a(w * 0.5 / r.self()); break;
    case OP_SQR: r.add_a(w * 2.0 * r.a()); break;
    // (1 - a)(1 + a), not 1 - a a: both factors are exact near |a| = 1, where a a rounds by as much as is left of 1 - a a (half the digits of the slope at 1 - 1e-8, all of them at 1 - 1e-16)
    case OP_ASIN: { const double va = r.a(); r.add_a(w / sqrt((1.0 - va) * (1.0 + va))); } break;
    case OP_FABS: { const double va = r.a(); r.add_a(w * (va > 0.0 ? 1.0 : (va < 0.0 ? -1.0 : 0.0))); } break;
    case OP_FMIN: if (r.a() <= r.b()) r.add_a(w); else r.add_b(w); break;  // casadi: d fmin = (x <= y, !(x <= y))
    case OP_FMAX: if (r.a() >= r.b()) r.add_a(w); else r.add_b(w); break;
    case OP_IFZ: if (r.a() != 0.0) r.add_b(w); break;
    case OP_EXP: r.add_a(w * r.self()); break;
    case OP_LOG: r.add_a(w / r.a()); break;
    default: break;
  }
}

#endif  // OH_TAPE_OPS_H
