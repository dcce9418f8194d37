// Runs the postfix programs of wxa::host::Parser (host/Parser.hpp) on the device, with Parser::eval's semantics:
// `if` is a select (both arms have been evaluated), power() multiplies repeatedly for integer exponents with
// |b| <= 16, heaviside(0, b) = b, min / max are the a < b ? a : b forms; one rounding per operation.
//
// The program is the same for every lane of a launch, so the lanes of a wave step through it together: the op is
// fetched with scalar loads and every branch on it is uniform.  Only the value stack is per lane.  Its top lives in a
// register, the rest in LDS laid out [depth][thread] -- a wave's access at one depth is 64 consecutive doubles -- and
// not in a private array, which the run-time stack pointer would send to scratch memory.
#ifndef WXA_EXPR_DEVICE_HPP_
#define WXA_EXPR_DEVICE_HPP_

#include <vector>

#include "common.hpp"
#include "host/ExprHandle.hpp"

#define WXA_EXPR_MAX_DEPTH 16    // values on the stack at once
#define WXA_EXPR_MAX_OPS 256     // operations of one program
#define WXA_EXPR_BLOCK 256       // work-items per workgroup of every kernel that evaluates programs

namespace wxa {

struct ExprOp {
    int32_t code, arg;   // Parser::Code; the variable's index (VAR) or the function's id (F1, F2)
    double value;        // NUM
};
// one program inside a buffer of ExprOp
struct ExprProg {
    const ExprOp* ops;
    int n;
};

// LDS of a kernel that evaluates programs: `__shared__ double stack[WXA_EXPR_STACK_DOUBLES]`, column threadIdx.x.
// The top of the stack is a register, so WXA_EXPR_MAX_DEPTH values need one row less.
#define WXA_EXPR_STACK_DOUBLES ((WXA_EXPR_MAX_DEPTH - 1) * WXA_EXPR_BLOCK)

__device__ __forceinline__ double expr_power(double a, double b) {
#pragma clang fp contract(off)
    if (b == floor(b) && fabs(b) <= 16.0) {
        int n = (int)fabs(b);
        double r = 1.0, x = a;
        while (n) { if (n & 1) r *= x; x *= x; n >>= 1; }
        return b < 0 ? 1.0 / r : r;
    }
    return pow(a, b);
}

__device__ __forceinline__ double expr_call1(int id, double a) {
    using P = host::Parser;
    switch (id) {
        case P::SQRT: return sqrt(a);   case P::EXP: return exp(a);     case P::LOG: return log(a);
        case P::LOG10: return log10(a); case P::SIN: return sin(a);     case P::COS: return cos(a);
        case P::TAN: return tan(a);     case P::ASIN: return asin(a);   case P::ACOS: return acos(a);
        case P::ATAN: return atan(a);   case P::SINH: return sinh(a);   case P::COSH: return cosh(a);
        case P::TANH: return tanh(a);   case P::ABS: return fabs(a);    case P::FLOOR: return floor(a);
        case P::CEIL: return ceil(a);   case P::ERF: return erf(a);
    }
    return 0.0;
}

__device__ __forceinline__ double expr_call2(int id, double a, double b) {
    using P = host::Parser;
    switch (id) {
        case P::FPOW: return expr_power(a, b); case P::ATAN2: return atan2(a, b);
        case P::FMIN: return a < b ? a : b;    case P::FMAX: return a > b ? a : b;
        case P::FMOD: return fmod(a, b);
        case P::HEAVISIDE: return a < 0.0 ? 0.0 : (a > 0.0 ? 1.0 : b);
    }
    return 0.0;
}

// The value of `prog` for this lane.  `col` = the lane's column of the LDS stack (stack + threadIdx.x); load(i) = the
// lane's value of variable i.  Every lane of the workgroup may call it (none waits for another: no barrier inside);
// a lane without a point of its own passes any finite values and drops the result.
template <class Load>
__device__ __forceinline__ double expr_run(const ExprProg prog, double* __restrict__ col, Load load) {
#pragma clang fp contract(off)
    using P = host::Parser;
    double top = 0.0;
    int sp = 0;   // values on the stack: `top` and col[0 .. sp - 2]
    for (int i = 0; i < prog.n; ++i) {
        const ExprOp op = prog.ops[i];
        switch (op.code) {
            case P::NUM:
            case P::VAR:
                if (sp > 0) col[(sp - 1) * WXA_EXPR_BLOCK] = top;
                top = op.code == P::NUM ? op.value : load(op.arg);
                ++sp;
                break;
            case P::NEG: top = -top; break;
            case P::F1: top = expr_call1(op.arg, top); break;
            case P::IF: {
                const double c = col[(sp - 3) * WXA_EXPR_BLOCK], a = col[(sp - 2) * WXA_EXPR_BLOCK];
                top = c != 0.0 ? a : top;
                sp -= 2;
                break;
            }
            default: {
                const double a = col[(sp - 2) * WXA_EXPR_BLOCK], b = top;
                switch (op.code) {
                    case P::ADD: top = a + b; break;
                    case P::SUB: top = a - b; break;
                    case P::MUL: top = a * b; break;
                    case P::DIV: top = a / b; break;
                    case P::POW: top = expr_power(a, b); break;
                    case P::LT: top = a < b ? 1.0 : 0.0; break;
                    case P::GT: top = a > b ? 1.0 : 0.0; break;
                    case P::LE: top = a <= b ? 1.0 : 0.0; break;
                    case P::GE: top = a >= b ? 1.0 : 0.0; break;
                    case P::EQ: top = a == b ? 1.0 : 0.0; break;
                    case P::NE: top = a != b ? 1.0 : 0.0; break;
                    case P::AND: top = (a != 0.0 && b != 0.0) ? 1.0 : 0.0; break;
                    case P::OR: top = (a != 0.0 || b != 0.0) ? 1.0 : 0.0; break;
                    case P::F2: top = expr_call2(op.arg, a, b); break;
                    default: break;
                }
                --sp;
            }
        }
    }
    return top;
}

// ---- host side ----
// `what` names the expression in the message ("the density expression"); false + last error if the program is
// beyond what expr_run's stack and the program buffers take
inline bool expr_fits_device(const wxa_expr* e, const char* entry, const char* what) {
    const int n = (int)e->parser.program().size(), depth = e->parser.depth();
    if (n < 1) { set_last_error("%s: %s is empty", entry, what); return false; }
    if (n > WXA_EXPR_MAX_OPS) {
        set_last_error("%s: %s has %d operations, the device evaluator takes at most %d", entry, what, n, WXA_EXPR_MAX_OPS);
        return false;
    }
    if (depth > WXA_EXPR_MAX_DEPTH) {
        set_last_error("%s: %s needs a value stack of depth %d, the device evaluator has %d", entry, what, depth,
                       WXA_EXPR_MAX_DEPTH);
        return false;
    }
    return true;
}
inline void expr_serialise(const wxa_expr* e, std::vector<ExprOp>& out) {
    for (const host::Parser::Op& op : e->parser.program()) out.push_back(ExprOp{(int32_t)op.code, (int32_t)op.arg, op.value});
}

}  // namespace wxa
#endif
