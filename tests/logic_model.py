"""The model of the comparator, bitwise, byte-order and const-arithmetic maps (csrc/logic.hip), for the tests.

numpy's operators on the typed arrays ARE the C++ operators of the reference's loops for these maps: comparisons (a NaN makes every
ordered comparison and == false and != true, -0.0 == 0.0), `~ & | ^`, left_shift / right_shift below the bit width (the low bits
kept; arithmetic for the signed types, logical for the unsigned ones) and .byteswap() of the scalar view.  tests/test_logic_cpu.py
holds every one of them to what g++ recorded in tests/golden/logic.npz.  Arithmetic with a constant is oracle.arith with one operand
broadcast, the model /comms/arithmetic is held to.
"""
import functools

import numpy as np

CMP = {">": "GT", "<": "LT", ">=": "GE", "<=": "LE", "==": "EQ", "!=": "NE"}                      # device.CMP_OPS -> fixture names
ARITHK = {"X+K": "ADDK", "X-K": "SUBK", "K-X": "KSUB", "X*K": "MULK", "X/K": "DIVK", "K/X": "KDIV"}  # device.ARITHK_OPS -> fixture names
INT_TYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"]
TYPES = INT_TYPES + ["float32", "float64"]

_CMP_FN = {">": np.greater, "<": np.less, ">=": np.greater_equal, "<=": np.less_equal, "==": np.equal, "!=": np.not_equal}
_BIT_FN = {"AND": np.bitwise_and, "OR": np.bitwise_or, "XOR": np.bitwise_xor}


def compare(op, a, b):
    """b: an array like a, or one element of a's type"""
    a = np.asarray(a)
    return _CMP_FN[op](a, np.asarray(b, dtype=a.dtype)).astype(np.uint8)


def bitwise(op, ins):
    if op == "NOT":
        (a,) = ins
        return np.invert(a)
    return functools.reduce(_BIT_FN[op], ins)


def bitwise_const(op, x, k):
    return _BIT_FN[op](x, np.asarray(k, dtype=x.dtype).reshape(-1)[0])


def bitshift(left, x, shift):
    assert 0 <= shift < 8 * x.dtype.itemsize
    return (np.left_shift if left else np.right_shift)(x, x.dtype.type(shift))


def byteswap(x):
    """every scalar reversed; a complex element is two scalars"""
    x = np.ascontiguousarray(x)
    if x.dtype.kind == "c":
        return x.view(x.real.dtype).byteswap().view(x.dtype)
    return x.byteswap()


def arith_const(oracle, op, x, k, cplx):
    """x: (n,) or, complex, (n, 2); k: one element of the type"""
    kb = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=x.dtype).reshape(-1), x.shape))
    code = {"+": oracle.ADD, "-": oracle.SUB, "*": oracle.MUL, "/": oracle.DIV}[op[1]]
    return oracle.arith(code, kb, x, cplx) if op[0] == "K" else oracle.arith(code, x, kb, cplx)
