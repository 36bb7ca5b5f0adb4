"""The generated multiplier instruction streams (csrc/gen_mul28_asm.py -> gs_mul28_asm.h) interpreted on the CPU over the
contract-limit operands of tests/arithvec.py.

The CPU twin replaces these bodies by C++ (`*_generic`), and on the device they only ever see random witnesses, whose
column sums sit near half of the worst case.  Here `Machine` (tests/test_pointops_gen.py: the generators' opcodes on
Python integers, a 64-bit accumulator that leaves int64 or a lazy 32-bit sum that leaves int32 is an AssertionError) runs

    sub_body(L, False)   product          a v0..    b vL..                       -> v2L..
    sub_body(L, True)    squaring         a v0..    (vL.. destroyed: 2a)          -> v2L..
    sub_body_fp2(L)      Fp2 product      a0 a1 b0 b1 at v0, vL, v2L, v3L         -> v4L.., v5L..
    sub_body_fp2sqr(L)   Fp2 squaring     a0 a1 at v0, vL                         -> v2L.., v3L..
    sub_body_fp2dot(L,3) Fp2 dot product  pair t at v(4tL)..                      -> v12L.., v13L..

standalone for L = 14 and 10, and the INLINE forms gen(L) / gen_sqr(L) (what the GS_NO_ASM_CALL fallback build runs) with
their %-operands substituted by registers -- they need no opcode `Machine` lacks, so they are covered here as well as by
the second build of tests/test_gpu_arith.py.  Every result is compared with big integers: the limbs are EXACTLY those of
(W + m p) / 2^(28L) for the exact double-length W (so: congruent, limbs 0..L-2 in [0, 2^28), value in [W/R, W/R + p), which
is inside (-p/2, 3p/2) whenever |W| < R p / 2); the registers a body declares preserved are unchanged and those it declares
destroyed are the only others written.  Cases: every extreme and edge case (a sixth of the 1 100 edge PAIRS of the single
product) and 40 of the random ones per body; the full random sets run in the twin and on the device, where they are cheap.
One negative control per body: one operand one step over the contract must trip an assertion.  No GPU needed."""
import re

import pytest

import arithvec as av
from test_pointops_gen import Machine, mulgen

CURVES = [("bls12_381", 14), ("bn254", 10)]


def _layout(body, L):
    """(program, input bases, output bases, registers the body may destroy)"""
    if body == "mul":
        return mulgen.sub_body(L, False), [0, L], [2 * L], range(3 * L, 3 * L + 3)
    if body == "sqr":
        return mulgen.sub_body(L, True), [0], [2 * L], list(range(L, 2 * L)) + list(range(3 * L, 3 * L + 3))
    if body == "fp2mul":
        return mulgen.sub_body_fp2(L), [0, L, 2 * L, 3 * L], [4 * L, 5 * L], range(6 * L, 7 * L + 4)
    if body == "fp2sqr":
        return mulgen.sub_body_fp2sqr(L), [0, L], [2 * L, 3 * L], range(4 * L, 7 * L + 4)
    return mulgen.sub_body_fp2dot(L, 3), [q * L for q in range(12)], [12 * L, 13 * L], range(14 * L, 17 * L + 4)


def _inline(body, L):
    """the inline asm block of gen(L) / gen_sqr(L) as a program on registers: r = v80.., a = v40.., b (or d = 2a) = v60..,
    modulus in s40.. as for the subroutines; v32..v34 are the block's own scratch"""
    src = (mulgen.gen if body == "mul" else mulgen.gen_sqr)(L)[0]
    text = src.split('asm("', 1)[1].split('"\n', 1)[0]

    def reg(m):
        k = int(m.group(1))
        if k < L:
            return "v%d" % (80 + k)
        if k < 2 * L:
            return "v%d" % (40 + k - L)
        if k < 3 * L:
            return "v%d" % (60 + k - 2 * L)
        return "s%d" % (40 + k - 3 * L)

    prog = [re.sub(r"%(\d+)", reg, ins) for ins in text.split("\\n\\t")]
    assert len(prog) > 2 * L * L // 2 and not any("%" in x for x in prog)
    return prog, [40, 60], [80], range(32, 35)


def _run(c, body, ops, layout):
    prog, ins, outs, scratch = layout
    L = c.L
    m = Machine(c.p, L)
    for base, o in zip(ins, ops):
        for i, x in enumerate(o):
            m.v[base + i] = x
    before = dict(m.v)
    others = (dict(m.s), dict(m.a), dict(m.sflag))
    m.run(prog)
    # SGPRs (the modulus, the G2 filter's constant: live values of the point programs that call these bodies), AGPRs and
    # the scalar flags: a multiplier body writes none of them (it declares vcc and its return address s[34:35] only)
    assert (m.s, m.a, m.sflag) == others, "a scalar or accumulation register was written"
    allowed = set(before) | {b + i for b in outs for i in range(L)} | set(scratch)
    destroyed = set(scratch)
    assert set(m.v) <= allowed, sorted(set(m.v) - allowed)
    assert all(m.v[k] == x for k, x in before.items() if k not in destroyed), "a preserved register changed"
    return [[m.v[b + i] for i in range(L)] for b in outs]


def _check(c, body, ops, got, name):
    want = av.exact(c, body, ops)
    assert got == want, (body, name)
    for r in got:  # what the equality implies, spelled out as the header states it
        assert all(0 <= x < (1 << 28) for x in r[:-1]), (body, name)


def _subset(cname, body):
    n_edge = n_rand = 0
    for case in av.multiplier_cases(cname):
        if case.body != body:
            continue
        if case.kind == "edge" and body == "mul":
            n_edge += 1
            if n_edge % 6:
                continue
        if case.kind == "random":
            n_rand += 1
            if n_rand > 40:
                continue
        yield case


@pytest.mark.parametrize("cname,L", CURVES)
def test_operand_sets_prove_their_labels(cname, L):
    """every vector inside its contract, every extreme label reached exactly, the docstring's figures"""
    av.selfcheck(cname)


@pytest.mark.parametrize("body", av.BODIES)
@pytest.mark.parametrize("cname,L", CURVES)
def test_subroutine_bodies_at_contract_limits(cname, L, body):
    c = av.ctx(cname)
    layout = _layout(body, L)
    n = 0
    for case in _subset(cname, body):
        got = _run(c, body, case.ops, layout)
        _check(c, body, case.ops, got, case.name)
        if case.tier == 2 and case.kind == "random":
            # operands that are lazy sums of products (|V| a few p): the output interval of the header
            for r in got:
                if max(abs(c.val(o)) for o in case.ops) ** 2 * 6 < c.R * c.p // 2:
                    assert -c.p // 2 < c.val(r) < 3 * c.p // 2, case.name
        n += 1
    assert n >= 40 + 4


@pytest.mark.parametrize("body", ["mul", "sqr"])
@pytest.mark.parametrize("cname,L", CURVES)
def test_inline_forms_at_contract_limits(cname, L, body):
    """gen(L) / gen_sqr(L): the blocks the GS_NO_ASM_CALL build inlines.  The squaring takes d = 2a from its caller."""
    c = av.ctx(cname)
    layout = _inline(body, L)
    for case in _subset(cname, body):
        ops = case.ops if body == "mul" else [case.ops[0], [2 * x for x in case.ops[0]]]
        assert av.s32ok(ops[-1])
        got = _run(c, body, ops, layout)
        _check(c, body, case.ops, got, case.name)


@pytest.mark.parametrize("body", av.BODIES)
@pytest.mark.parametrize("cname,L", CURVES)
def test_one_step_over_the_contract_trips_an_assertion(cname, L, body):
    """negative control: the interpreter's width assertions are looking.  The same extreme case with one operand's limbs
    doubled leaves int64 (or int32, in the squarings' operand sums)."""
    c = av.ctx(cname)
    case = av.over_contract_case(cname, body)
    with pytest.raises(AssertionError, match="overflow|wrapped"):
        _run(c, body, case.ops, _layout(body, L))
    if body == "mul":
        with pytest.raises(AssertionError, match="overflow|wrapped"):
            _run(c, body, case.ops, _inline(body, L))
    if body == "sqr":  # the inline squaring takes d = 2a from its caller: that doubling is what leaves int32 here
        assert not av.s32ok([2 * x for x in case.ops[0]])
