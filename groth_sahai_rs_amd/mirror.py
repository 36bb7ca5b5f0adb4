"""Host-side mirror of the reference's operator interface for the hot path, on
top of the C ABI (same names, argument meaning and error behaviour):

    CRS, generate_crs                     src/generator.rs:35-42, 81-118 (generators supplied by the caller)
    Commit1 / Commit2 {coms, rand}        src/prover/commit.rs:18-28
    batch_commit_G1 / _G2 / _scalar_to_B1 / _scalar_to_B2, commit_G1 ...   commit.rs:59-256
    PPE / MSMEG1 / MSMEG2 / QuadEqu {a_consts, b_consts, gamma, target}     src/statement.rs:117-192
        .commit_and_prove(xvars, yvars, crs, rng) -> CProof                src/prover/prove.rs:29-52
        .prove(xvars, yvars, xcoms, ycoms, crs, rng) -> EquProof
        .verify(com_proof, crs) -> bool                                    src/verifier.rs:18-21
        .evaluate(xvars, yvars, crs) -> target, .is_satisfied_by(xvars, yvars, crs) -> bool, <Type>.from_witness(..)
                                                                           (new) the left-hand side at a witness
    rerandomize(equ, com_proof, crs, rng) -> CProof                      (new) fresh commitments and proof, no witness
    generate_crs_with_key -> (CRS, key), extract(commit, crs, key)        (new) open commitments with the binding key
    extract_scalars(commit, crs, key, bits, log2_table=None)              (new) committed scalars < 2^bits back themselves
    generate_crs_with_trapdoor -> (hiding CRS, trapdoor), <Equation>.simulate(crs, trapdoor, rng), Statement.simulate,
    equivocate(x, r, x_new, t)                                            (new) proofs without a witness, hiding CRS
    DeviceRng(engine, key)                                                (new) as `rng`: R, S, T are drawn on the device
    EquProof {pi, theta, equ_type, rand}, CProof {xcoms, ycoms, equ_proofs} prove.rs:55-69

Values are numpy uint64 limb arrays in the boundary layout of include/gs_amd.h
(G1 = 2*NQ limbs, G2 = 4*NQ, Fr = 4, GT = 12*NQ); lists of them where the
reference has Vec<..>.  `rng` is any object with a method fr() returning one
Montgomery-form scalar (4 u64 limbs); draws happen in the reference's order
(R row-major, then S, then T: commit.rs:85-88,185-188; prove.rs:123-126).
Shape mismatches raise AssertionError where the reference panics via
assert_eq! (prove.rs:106-113; verifier.rs:25-26).

The batched entry points (`prove_many` / `verify_many`) are the build's
addition: N independent equations of one shape over the shared CRS -- the
reference has no batch API.
"""
import numpy as np

from .capi import GS_MSMEG1, GS_MSMEG2, GS_PPE, GS_QUAD, Engine


class CRS:
    """u: [Com1;2], v: [Com2;2], g1_gen, g2_gen, gt_gen  (generator.rs:35-42)."""

    def __init__(self, u, v, g1_gen, g2_gen, gt_gen, curve=0, device=0):
        self.u, self.v, self.g1_gen, self.g2_gen, self.gt_gen = u, v, g1_gen, g2_gen, gt_gen
        self.engine = Engine(curve, device)
        flat = np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in (u[0], u[1], v[0], v[1], g1_gen,
                                                                                   g2_gen, gt_gen)])
        self.engine.set_crs(flat)


def _crs_from_scalars(p1, p2, sc, curve, device, hiding):
    eng = Engine(curve, device)
    raw = eng.crs_generate(p1, p2, sc, hiding=hiding).view(np.uint64)  # hiding: generator.rs:65-77
    eng.close()
    g1, g2 = eng.G1 // 8, eng.G2 // 8
    o = 0
    parts = []
    for sz in (2 * g1, 2 * g1, 2 * g2, 2 * g2, g1, g2, eng.GT // 8):
        parts.append(raw[o:o + sz].copy())
        o += sz
    return CRS([parts[0], parts[1]], [parts[2], parts[3]], parts[4], parts[5], parts[6], curve, device)


def generate_crs(p1, p2, rng, curve=0, device=0, hiding=False):
    """AbstractCrs::generate_crs (generator.rs:81-118) with the group generators supplied by the caller
    (the reference draws them with G1::rand / G2::rand, which has no counterpart outside arkworks);
    the four scalars a1, a2, t1, t2 are drawn from `rng` in the reference's order (generator.rs:90-93)."""
    sc = np.concatenate([rng.fr() for _ in range(4)])
    return _crs_from_scalars(p1, p2, sc, curve, device, hiding)


def generate_crs_with_key(p1, p2, rng, curve=0, device=0, hiding=False):
    """generate_crs that also hands out the binding key: (CRS, key), key = a1 || a2 (8 u64 limbs, Montgomery form).
    The draws are those of generate_crs, so the same rng state gives the same CRS.  The key opens every commitment
    made under this CRS (extract below): keep it secret, or drop it."""
    sc = np.concatenate([rng.fr() for _ in range(4)])
    return _crs_from_scalars(p1, p2, sc, curve, device, hiding), sc[:8].copy()


def generate_crs_with_trapdoor(p1, p2, rng, curve=0, device=0):
    """The HIDING CRS (generator.rs:65-77) together with its simulation trapdoor: (CRS, trapdoor), trapdoor = t1 || t2
    (8 u64 limbs, Montgomery form).  The draws are those of generate_crs, so the same rng state gives the same CRS as
    generate_crs(.., hiding=True).  The trapdoor answers every equation without a witness (equ.simulate below) and opens
    a scalar commitment to any value (equivocate): keep it secret, or drop it."""
    sc = np.concatenate([rng.fr() for _ in range(4)])
    return _crs_from_scalars(p1, p2, sc, curve, device, True), sc[8:16].copy()


def equivocate(x, r, x_new, t, curve=0):
    """The randomness that opens the hiding scalar commitment c = x W + r key0 (commit_scalar_to_B1 / _B2 under a CRS of
    generate_crs_with_trapdoor) to x_new instead: r + (x - x_new) t, since W = t key0 there.  t is the trapdoor scalar of
    the commitment's side (t1 for B1, t2 for B2).  All values are Montgomery Fr limbs; host Fr arithmetic, no GPU."""
    q = _FR_ORDER[curve]
    return _fr_limbs((_fr_int(r, q) + (_fr_int(x, q) - _fr_int(x_new, q)) * _fr_int(t, q)) % q, q)


def extract(commit, crs, key):
    """What the commitments of a Commit1 / Commit2 bind, opened with the binding key of `crs`: c.1 - a c.0 for each
    (gs_extract_g1 / gs_extract_g2).  A committed group element comes back itself; a committed scalar x comes back as
    x * generator (its image: x itself is a discrete logarithm away).  Raises GsError (code 3) when `key` is not the
    binding key of `crs`, in particular on a hiding CRS.  The key stays installed in crs.engine until
    crs.engine.set_extraction_key(None)."""
    group = 2 if isinstance(commit, Commit2) else 1
    crs.engine.set_extraction_key(key)
    n = len(commit.coms)
    if n == 0:
        return []
    out = crs.engine.extract(group, _cat(commit.coms, 0))
    return [out[i].view(np.uint64).copy() for i in range(n)]


def extract_scalars(commit, crs, key, bits, log2_table=None):
    """The scalars a Commit1 / Commit2 of batch_commit_scalar_to_B1 / _B2 binds, opened with the binding key of `crs`:
    a list with the Fr (Montgomery limbs, as it was committed) of every scalar below 2^bits and None where there is none
    (gs_extract_scalar_b1 / _b2: extraction, then a baby-step giant-step walk from the image x * generator back to x).
    The baby-step table of the group, 2^log2_table multiples of crs.g1_gen / crs.g2_gen, is built unless the last
    dlog_prepare of crs.engine for the group was for exactly this base and size (Engine.dlog_prepare records both);
    log2_table = None picks about half of bits (at most 24, at least 2 and what keeps a lane's walk below 2^24 steps),
    so calls that alternate between values of bits rebuild the table unless they pass one log2_table.  Raises GsError
    as extract does."""
    group = 2 if isinstance(commit, Commit2) else 1
    crs.engine.set_extraction_key(key)
    if log2_table is None:
        log2_table = max(2, min(24, (bits + 1) // 2), bits - 25)
    base = crs.g1_gen if group == 1 else crs.g2_gen
    if crs.engine.dlog_table(group) != (np.ascontiguousarray(base).view(np.uint8).tobytes(), int(log2_table)):
        crs.engine.dlog_prepare(group, base, log2_table)
    n = len(commit.coms)
    if n == 0:
        return []
    xs, found = crs.engine.extract_scalar(group, _cat(commit.coms, 0), bits)
    return [xs[i].view(np.uint64).copy() if found[i] else None for i in range(n)]


class DeviceRng:
    """Randomness drawn ON the device (include/gs_amd.h, "randomness drawn on the device"): installs the 32-byte
    ChaCha20 `key` in `engine` and hands out stream numbers 0, 1, 2, ... -- one per call, as the contract demands (a
    reused (key, stream) pair repeats the randomness and links the proofs).  Given as `rng` to
    <Equation>.commit_and_prove, Statement.commit_and_prove or rerandomize, the call goes through the drawn entry
    (gs_prove_batch_drawn, gs_prove_statement_drawn, gs_rerandomize_batch_drawn): R, S, T are generated in device
    memory and come back with the proof, so the returned objects carry them like any other.  The results are NOT the
    reference's for any rng state; with any other rng nothing changes.  The key must come from a CSPRNG."""

    def __init__(self, engine, key, first_stream=0):
        self.engine, self.stream = engine, first_stream
        engine.rand_set_key(key)

    def next_stream(self):
        self.stream += 1
        return self.stream - 1

    def _for(self, crs):
        assert crs.engine is self.engine, "the DeviceRng's key is installed in another engine than the CRS's"
        return self.next_stream()


def _mat(buf, rows, cols):
    """flat Montgomery scalars -> Matrix<Fr> as the mirror objects hold it"""
    a = np.asarray(buf).view(np.uint64).reshape(rows, cols, 4)
    return [[a[i, j].copy() for j in range(cols)] for i in range(rows)]


class Commit1:
    def __init__(self, coms, rand):
        self.coms, self.rand = coms, rand  # coms: list of Com1 (4*NQ limbs); rand: Matrix<Fr>

    def __eq__(self, o):
        return all((a == b).all() for a, b in zip(self.coms, o.coms)) and _mat_eq(self.rand, o.rand)

    def append(self, other):  # commit.rs:43-51
        assert len(self.coms) == len(self.rand) and len(other.coms) == len(other.rand)
        self.coms += other.coms
        self.rand += other.rand
        other.coms, other.rand = [], []


class Commit2(Commit1):
    pass


def _mat_eq(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all((p == q).all() for p, q in zip(x, y)) for x, y in zip(a, b))


def _cat(xs, width):
    if len(xs) == 0:
        return np.zeros(0, dtype=np.uint64)
    return np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in xs])


def _flat_mat(m):
    return _cat([e for row in m for e in row], 4)


def _split(buf, n):
    a = np.asarray(buf).view(np.uint64)
    return [a[i * (a.size // n):(i + 1) * (a.size // n)].copy() for i in range(n)] if n else []


def _batch_commit(kind, vars_, key, rng, cols):
    n = len(vars_)
    rand = [[rng.fr() for _ in range(cols)] for _ in range(n)]
    if n == 0:
        return [], rand
    out = key.engine.commit(kind, _cat(vars_, 0), _flat_mat(rand))
    return [out[i].view(np.uint64).copy() for i in range(n)], rand


def batch_commit_G1(xvars, key, rng):  # commit.rs:78-100
    return Commit1(*_batch_commit("g1", xvars, key, rng, 2))


def batch_commit_G2(yvars, key, rng):  # commit.rs:178-200
    return Commit2(*_batch_commit("g2", yvars, key, rng, 2))


def batch_commit_scalar_to_B1(scalar_xvars, key, rng):  # commit.rs:125-156
    return Commit1(*_batch_commit("fr_b1", scalar_xvars, key, rng, 1))


def batch_commit_scalar_to_B2(scalar_yvars, key, rng):  # commit.rs:225-256
    return Commit2(*_batch_commit("fr_b2", scalar_yvars, key, rng, 1))


def commit_G1(xvar, key, rng):  # commit.rs:59-75
    return batch_commit_G1([xvar], key, rng)


def commit_G2(yvar, key, rng):
    return batch_commit_G2([yvar], key, rng)


def commit_scalar_to_B1(x, key, rng):
    return batch_commit_scalar_to_B1([x], key, rng)


def commit_scalar_to_B2(y, key, rng):
    return batch_commit_scalar_to_B2([y], key, rng)


class EquProof:
    def __init__(self, pi, theta, equ_type, rand):
        self.pi, self.theta, self.equ_type, self.rand = pi, theta, equ_type, rand


class CProof:
    def __init__(self, xcoms, ycoms, equ_proofs):
        self.xcoms, self.ycoms, self.equ_proofs = xcoms, ycoms, equ_proofs


class _Equation:
    TYPE = None

    def __init__(self, a_consts, b_consts, gamma, target):
        self.a_consts, self.b_consts, self.gamma, self.target = a_consts, b_consts, gamma, target

    def get_type(self):
        return self.TYPE

    def _check_statement_shape(self, m, n):
        """a_consts pair with the n Y variables, b_consts with the m X variables, Gamma is m x n."""
        assert len(self.a_consts) == n, "a_consts.len() == yvars.len()"
        assert len(self.b_consts) == m, "b_consts.len() == xvars.len()"
        assert len(self.gamma) == m and all(len(row) == n for row in self.gamma), "gamma is m x n"

    # -- evaluation (the left-hand sides of statement.rs:17-21) ---------------
    def evaluate(self, xvars, yvars, crs):
        """What the equation evaluates to at the witness (gs_eval_batch): a GT / G1 / G2 / Fr value in the limbs `target`
        is held in -- the target that makes (xvars, yvars) a satisfying witness.  The reference leaves this sum to the
        caller (tests/prover.rs:50-52 writes it out with arkworks)."""
        m, n = len(xvars), len(yvars)
        assert m >= 1 and n >= 1
        self._check_statement_shape(m, n)
        out = crs.engine.eval_batch(self.TYPE, 1, m, n, _cat(xvars, 0), _cat(yvars, 0), _cat(self.a_consts, 0),
                                    _cat(self.b_consts, 0), _flat_mat(self.gamma))
        return out[0].view(np.uint64).copy()

    def is_satisfied_by(self, xvars, yvars, crs):
        """Does the witness satisfy the equation -- does it evaluate to `target` (gs_check_witness_batch)?  What
        Provable::prove never checks: a proof made from a wrong witness fails only at the verifier."""
        m, n = len(xvars), len(yvars)
        assert m >= 1 and n >= 1
        self._check_statement_shape(m, n)
        ok = crs.engine.check_witness_batch(self.TYPE, 1, m, n, _cat(xvars, 0), _cat(yvars, 0), _cat(self.a_consts, 0),
                                            _cat(self.b_consts, 0), _flat_mat(self.gamma),
                                            np.asarray(self.target, dtype=np.uint64).reshape(-1))
        return bool(ok[0])

    @classmethod
    def from_witness(cls, a_consts, b_consts, gamma, xvars, yvars, crs):
        """The equation with these constants whose target is its value at (xvars, yvars): true by construction."""
        equ = cls(a_consts, b_consts, gamma, None)
        equ.target = equ.evaluate(xvars, yvars, crs)
        return equ

    # -- Provable ---------------------------------------------------------
    def _kxky(self):
        return (2 if self.TYPE in (GS_PPE, GS_MSMEG1) else 1), (2 if self.TYPE in (GS_PPE, GS_MSMEG2) else 1)

    def commit_and_prove(self, xvars, yvars, crs, rng):  # prove.rs:72-90 etc.
        kx, ky = self._kxky()
        if isinstance(rng, DeviceRng):
            return Statement([self]).commit_and_prove(xvars, yvars, crs, rng)  # (E = 1: the same draws, the same bytes)
        xcoms = (batch_commit_G1 if kx == 2 else batch_commit_scalar_to_B1)(xvars, crs, rng)
        ycoms = (batch_commit_G2 if ky == 2 else batch_commit_scalar_to_B2)(yvars, crs, rng)
        return CProof(xcoms, ycoms, [self.prove(xvars, yvars, xcoms, ycoms, crs, rng)])

    def prove(self, xvars, yvars, xcoms, ycoms, crs, rng):  # prove.rs:92-171 etc.
        kx, ky = self._kxky()
        # the reference's shape asserts (prove.rs:106-113)
        assert len(xvars) == len(xcoms.rand)
        assert len(self.gamma) == len(xcoms.rand)
        assert len(xcoms.rand[0]) == kx
        assert len(yvars) == len(ycoms.rand)
        assert len(self.gamma[0]) == len(ycoms.rand)
        assert len(ycoms.rand[0]) == ky
        m, n = len(xvars), len(yvars)
        self._check_statement_shape(m, n)
        assert all(len(r) == kx for r in xcoms.rand) and all(len(r) == ky for r in ycoms.rand)
        T = [[rng.fr() for _ in range(kx)] for _ in range(ky)]
        out = crs.engine.prove_batch(self.TYPE, 1, m, n, _cat(xvars, 0), _cat(yvars, 0), _cat(self.a_consts, 0),
                                     _cat(self.b_consts, 0), _flat_mat(self.gamma), _flat_mat(xcoms.rand),
                                     _flat_mat(ycoms.rand), _flat_mat(T), want_coms=False)
        pi, theta = _split(out["pi"], kx), _split(out["theta"], ky)
        assert len(pi) == kx and len(theta) == ky
        return EquProof(pi, theta, self.TYPE, T)

    # -- simulation (the hiding CRS's trapdoor; no witness) -------------------
    def simulate(self, crs, trapdoor, rng):
        """A CProof for this equation WITHOUT a witness (gs_simulate_batch), from the trapdoor of
        generate_crs_with_trapdoor: it verifies whatever the constants and the target are, and is distributed like an
        honest proof under that CRS.  Draws Rc (m x kx), then Sc (n x ky), then Tf (ky x kx) from `rng`; the commitments
        carry Rc / Sc as their `rand` (coordinates in the CRS basis: they open nothing), the proof carries Tf.  Refused
        for PPE (GsError code 3); raises GsError when `trapdoor` is not that of `crs`, in particular on a binding CRS.
        The trapdoor stays installed in crs.engine until crs.engine.set_simulation_key(None)."""
        return Statement([self]).simulate(crs, trapdoor, rng)

    # -- Verifiable --------------------------------------------------------
    def verify(self, com_proof, crs):  # verifier.rs:23-157
        assert len(com_proof.equ_proofs) == 1
        assert self.get_type() == com_proof.equ_proofs[0].equ_type
        pf = com_proof.equ_proofs[0]
        m, n = len(com_proof.xcoms.coms), len(com_proof.ycoms.coms)
        # proof lengths come from the wire: check them where the reference panics (pairing_sum / left_mul,
        # data_structures.rs:495,705) instead of letting the C ABI read past a short buffer
        kx, ky = self._kxky()
        assert m >= 1 and n >= 1
        self._check_statement_shape(m, n)
        assert len(pf.pi) == kx and len(pf.theta) == ky
        ok = crs.engine.verify_batch(self.TYPE, 1, m, n, _cat(self.a_consts, 0), _cat(self.b_consts, 0),
                                     _flat_mat(self.gamma), np.asarray(self.target, dtype=np.uint64),
                                     _cat(com_proof.xcoms.coms, 0), _cat(com_proof.ycoms.coms, 0), _cat(pf.pi, 0),
                                     _cat(pf.theta, 0))
        return bool(ok[0])


# scalar field orders (BLS12-381, BN254): the rand bookkeeping of rerandomize() is host-side Fr arithmetic on small
# matrices; Montgomery form with R = 2^256 (include/gs_amd.h)
_FR_ORDER = (0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
             0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001)


def _fr_int(v, r):  # Montgomery limbs -> canonical integer
    a = np.asarray(v, dtype=np.uint64).reshape(-1)
    return sum(int(a[i]) << (64 * i) for i in range(4)) * pow(1 << 256, -1, r) % r


def _fr_limbs(x, r):  # canonical integer -> Montgomery limbs
    y = (x << 256) % r
    return np.array([(y >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def rerandomize(equ, com_proof, crs, rng):
    """A fresh-looking CProof for `equ` from `com_proof` alone (gs_rerandomize_batch): no witness.  Draws R' (m x kx),
    then S' (n x ky), then T' (ky x kx) from `rng` -- the reference's draw order -- and returns commitments and proof
    that verify against the same equation and are distributed like a fresh proof of the same witness.  When the input
    carries its randomness (mirror objects always do), the result carries R + R', S + S' and T + T' + S'^T Gamma^T R:
    exactly what commit_and_prove with that randomness would have produced, byte for byte."""
    assert len(com_proof.equ_proofs) == 1
    pf = com_proof.equ_proofs[0]
    assert equ.get_type() == pf.equ_type
    kx, ky = equ._kxky()
    m, n = len(com_proof.xcoms.coms), len(com_proof.ycoms.coms)
    assert m >= 1 and n >= 1
    equ._check_statement_shape(m, n)
    # lengths that come from the wire are checked before a pointer crosses the C ABI
    assert len(pf.pi) == kx and len(pf.theta) == ky
    if isinstance(rng, DeviceRng):  # R', S', T' are drawn on the device and come back with the proof
        out = crs.engine.rerandomize_batch_drawn(equ.TYPE, 1, m, n, _cat(equ.a_consts, 0), _cat(equ.b_consts, 0),
                                                 _flat_mat(equ.gamma), _cat(com_proof.xcoms.coms, 0),
                                                 _cat(com_proof.ycoms.coms, 0), _cat(pf.pi, 0), _cat(pf.theta, 0),
                                                 rng._for(crs))
        R1, S1, T1 = _mat(out["R"], m, kx), _mat(out["S"], n, ky), _mat(out["T"], ky, kx)
    else:
        R1 = [[rng.fr() for _ in range(kx)] for _ in range(m)]
        S1 = [[rng.fr() for _ in range(ky)] for _ in range(n)]
        T1 = [[rng.fr() for _ in range(kx)] for _ in range(ky)]
        out = crs.engine.rerandomize_batch(equ.TYPE, 1, m, n, _cat(equ.a_consts, 0), _cat(equ.b_consts, 0),
                                           _flat_mat(equ.gamma), _cat(com_proof.xcoms.coms, 0),
                                           _cat(com_proof.ycoms.coms, 0), _cat(pf.pi, 0), _cat(pf.theta, 0),
                                           _flat_mat(R1), _flat_mat(S1), _flat_mat(T1))
    xr, yr, tr = com_proof.xcoms.rand, com_proof.ycoms.rand, pf.rand
    if xr is not None and yr is not None and tr is not None:
        r = _FR_ORDER[crs.engine.curve]
        I = lambda mat: [[_fr_int(v, r) for v in row] for row in mat]
        L = lambda mat: [[_fr_limbs(v, r) for v in row] for row in mat]
        R0, R1i, S0, S1i, T0, T1i, G = I(xr), I(R1), I(yr), I(S1), I(tr), I(T1), I(equ.gamma)
        xr = L([[(R0[i][a] + R1i[i][a]) % r for a in range(kx)] for i in range(m)])
        yr = L([[(S0[j][b] + S1i[j][b]) % r for b in range(ky)] for j in range(n)])
        # T'' = T + T' + S'^T Gamma^T R   (ky x kx)
        tr = L([[(T0[l][k] + T1i[l][k] + sum(S1i[j][l] * G[i][j] * R0[i][k] for i in range(m) for j in range(n))) % r
                 for k in range(kx)] for l in range(ky)])
    else:
        xr = yr = tr = None
    xcoms = Commit1(_split(out["xcoms"], m), xr)
    ycoms = Commit2(_split(out["ycoms"], n), yr)
    return CProof(xcoms, ycoms, [EquProof(_split(out["pi"], kx), _split(out["theta"], ky), equ.TYPE, tr)])


class PPE(_Equation):
    TYPE = GS_PPE


class MSMEG1(_Equation):
    TYPE = GS_MSMEG1


class MSMEG2(_Equation):
    TYPE = GS_MSMEG2


class QuadEqu(_Equation):
    TYPE = GS_QUAD


def _draw_rho(rng, count):
    """`count` non-zero 64-bit exponents for the batched verifiers from the caller's CSPRNG (the rho contract of
    gs_amd.h: fresh per call, secret until the verdict, drawn after the proofs are fixed).  Uses rng.u64() when the
    generator has one, else the low limb of a uniform scalar rng.fr(); a zero is drawn again."""
    out = np.zeros(count, dtype=np.uint64)
    for i in range(count):
        v = 0
        while v == 0:
            v = int(rng.u64()) if hasattr(rng, "u64") else int(np.asarray(rng.fr(), dtype=np.uint64).reshape(-1)[0])
        out[i] = v
    return out


def verify_batch_locate(equations, com_proofs, crs, rng):
    """[bool per equation] for INDEPENDENT equations of one type and shape, each with its own CProof (one EquProof),
    from the batched verifier with fault localisation (gs_verify_batch_rlc_locate): one combined check when the batch is
    valid, a descent of the kept product tree to the failing proofs when it is not.  True means "lies under a node
    whose combined check passed" (include/gs_amd.h): each such check errs with probability 2^-64 over rho, which is
    drawn here from `rng`."""
    N = len(equations)
    assert N >= 1 and len(com_proofs) == N
    ty = equations[0].TYPE
    kx, ky = equations[0]._kxky()
    m, n = len(com_proofs[0].xcoms.coms), len(com_proofs[0].ycoms.coms)
    assert m >= 1 and n >= 1
    for equ, cp in zip(equations, com_proofs):
        assert equ.TYPE == ty and len(cp.equ_proofs) == 1 and cp.equ_proofs[0].equ_type == ty
        assert len(cp.xcoms.coms) == m and len(cp.ycoms.coms) == n
        equ._check_statement_shape(m, n)
        assert len(cp.equ_proofs[0].pi) == kx and len(cp.equ_proofs[0].theta) == ky
    cat = np.concatenate
    ok, _, _ = crs.engine.verify_batch_rlc_locate(
        ty, N, m, n, cat([_cat(e.a_consts, 0) for e in equations]), cat([_cat(e.b_consts, 0) for e in equations]),
        cat([_flat_mat(e.gamma) for e in equations]),
        cat([np.asarray(e.target, dtype=np.uint64).reshape(-1) for e in equations]),
        cat([_cat(cp.xcoms.coms, 0) for cp in com_proofs]), cat([_cat(cp.ycoms.coms, 0) for cp in com_proofs]),
        cat([_cat(cp.equ_proofs[0].pi, 0) for cp in com_proofs]),
        cat([_cat(cp.equ_proofs[0].theta, 0) for cp in com_proofs]), _draw_rho(rng, 4 * N))
    return [bool(v) for v in ok]


def verify_equation_rlc(equation, com_proofs, crs, rng=None, rho=None):
    """ONE verdict for N CProofs (one EquProof each) of the SAME equation -- N showings of a credential, N ballots --
    from gs_verify_equation_rlc: the equation's constants cross the ABI once and the random linear combination is
    taken across the proofs before pairing.  True iff the combined check passes; a batch with a false proof passes with
    probability 2^-64 over rho, which is drawn here from the caller's CSPRNG `rng` unless `rho` (uint64[N * 4],
    non-zero; tests only) is given.  Which proofs of a failing batch are bad: verify_batch_locate."""
    N = len(com_proofs)
    assert N >= 1
    ty = equation.TYPE
    kx, ky = equation._kxky()
    m, n = len(com_proofs[0].xcoms.coms), len(com_proofs[0].ycoms.coms)
    assert m >= 1 and n >= 1
    equation._check_statement_shape(m, n)
    for cp in com_proofs:
        assert len(cp.equ_proofs) == 1 and cp.equ_proofs[0].equ_type == ty
        assert len(cp.xcoms.coms) == m and len(cp.ycoms.coms) == n
        assert len(cp.equ_proofs[0].pi) == kx and len(cp.equ_proofs[0].theta) == ky
    if rho is None:
        rho = _draw_rho(rng, 4 * N)
    cat = np.concatenate
    ok, _ = crs.engine.verify_equation_rlc(
        ty, N, m, n, _cat(equation.a_consts, 0), _cat(equation.b_consts, 0), _flat_mat(equation.gamma),
        np.asarray(equation.target, dtype=np.uint64).reshape(-1),
        cat([_cat(cp.xcoms.coms, 0) for cp in com_proofs]), cat([_cat(cp.ycoms.coms, 0) for cp in com_proofs]),
        cat([_cat(cp.equ_proofs[0].pi, 0) for cp in com_proofs]),
        cat([_cat(cp.equ_proofs[0].theta, 0) for cp in com_proofs]), rho)
    return bool(ok)


class Statement:
    """`pub type Statement = Vec<dyn Equ>` (statement.rs:109) made usable: a list of equations of ONE type over the same
    variables (statement.rs:24-28: "each equation is defined with respect to the list of variables that span across
    ALL equations").  The variables are committed once; every equation gets its own EquProof against those
    commitments -- exactly what batch_commit_* followed by `equ.prove(..)` per equation does in the reference, in
    one call of the engine (gs_prove_statement / gs_verify_statement).  RNG draw order: R, S, then T of equation 0, 1, ..
    """

    def __init__(self, equations):
        assert len(equations) >= 1 and all(e.TYPE == equations[0].TYPE for e in equations)
        self.equations = list(equations)
        self.TYPE = equations[0].TYPE

    def _kxky(self):
        return self.equations[0]._kxky()

    def commit_and_prove(self, xvars, yvars, crs, rng):
        kx, ky = self._kxky()
        m, n, E = len(xvars), len(yvars), len(self.equations)
        assert m >= 1 and n >= 1
        for equ in self.equations:
            equ._check_statement_shape(m, n)
        cat = np.concatenate
        consts = (cat([_cat(e.a_consts, 0) for e in self.equations]), cat([_cat(e.b_consts, 0) for e in self.equations]),
                  cat([_flat_mat(e.gamma) for e in self.equations]))
        if isinstance(rng, DeviceRng):  # R, S, T are drawn on the device and come back with the proofs
            out = crs.engine.prove_statement_drawn(self.TYPE, E, m, n, _cat(xvars, 0), _cat(yvars, 0), *consts,
                                                   rng._for(crs))
            R, S = _mat(out["R"], m, kx), _mat(out["S"], n, ky)
            Ts = [_mat(np.asarray(out["T"]).reshape(E, -1)[e], ky, kx) for e in range(E)]
        else:
            R = [[rng.fr() for _ in range(kx)] for _ in range(m)]
            S = [[rng.fr() for _ in range(ky)] for _ in range(n)]
            Ts = [[[rng.fr() for _ in range(kx)] for _ in range(ky)] for _ in range(E)]
            out = crs.engine.prove_statement(self.TYPE, E, m, n, _cat(xvars, 0), _cat(yvars, 0), *consts,
                                             _flat_mat(R), _flat_mat(S), cat([_flat_mat(T) for T in Ts]))
        xcoms = Commit1(_split(out["xcoms"], m), R)
        ycoms = Commit2(_split(out["ycoms"], n), S)
        pis, ths = _split(out["pi"], E * kx), _split(out["theta"], E * ky)
        proofs = [EquProof(pis[e * kx:(e + 1) * kx], ths[e * ky:(e + 1) * ky], self.TYPE, Ts[e]) for e in range(E)]
        return CProof(xcoms, ycoms, proofs)

    def simulate(self, crs, trapdoor, rng):
        """A CProof for the whole statement WITHOUT a witness (gs_simulate_statement): one simulated commitment set,
        one proof per equation.  Draw order: Rc, Sc, then Tf of equation 0, 1, ..  Refused for PPE."""
        kx, ky = self._kxky()
        E = len(self.equations)
        m, n = len(self.equations[0].b_consts), len(self.equations[0].a_consts)
        assert m >= 1 and n >= 1
        for equ in self.equations:
            equ._check_statement_shape(m, n)
        crs.engine.set_simulation_key(trapdoor)
        Rc = [[rng.fr() for _ in range(kx)] for _ in range(m)]
        Sc = [[rng.fr() for _ in range(ky)] for _ in range(n)]
        Ts = [[[rng.fr() for _ in range(kx)] for _ in range(ky)] for _ in range(E)]
        cat = np.concatenate
        out = crs.engine.simulate_statement(
            self.TYPE, E, m, n, cat([_cat(e.a_consts, 0) for e in self.equations]),
            cat([_cat(e.b_consts, 0) for e in self.equations]), cat([_flat_mat(e.gamma) for e in self.equations]),
            cat([np.asarray(e.target, dtype=np.uint64).reshape(-1) for e in self.equations]), _flat_mat(Rc),
            _flat_mat(Sc), cat([_flat_mat(T) for T in Ts]))
        pis, ths = _split(out["pi"], E * kx), _split(out["theta"], E * ky)
        proofs = [EquProof(pis[e * kx:(e + 1) * kx], ths[e * ky:(e + 1) * ky], self.TYPE, Ts[e]) for e in range(E)]
        return CProof(Commit1(_split(out["xcoms"], m), Rc), Commit2(_split(out["ycoms"], n), Sc), proofs)

    def _witness_arrays(self, xvars, yvars):
        """(m, n, X, Y, A, B, Gamma as gs_eval_statement takes them) after the shape checks"""
        m, n = len(xvars), len(yvars)
        assert m >= 1 and n >= 1
        for equ in self.equations:
            equ._check_statement_shape(m, n)
        cat = np.concatenate
        return m, n, (_cat(xvars, 0), _cat(yvars, 0), cat([_cat(e.a_consts, 0) for e in self.equations]),
                      cat([_cat(e.b_consts, 0) for e in self.equations]), cat([_flat_mat(e.gamma) for e in self.equations]))

    def evaluate(self, xvars, yvars, crs):
        """[the value of every equation at the shared witness] (gs_eval_statement): the targets that make it satisfying"""
        m, n, arrays = self._witness_arrays(xvars, yvars)
        out = crs.engine.eval_statement(self.TYPE, len(self.equations), m, n, *arrays)
        return [row.view(np.uint64).copy() for row in out]

    def is_satisfied_by(self, xvars, yvars, crs):
        """[bool per equation]: does the shared witness satisfy it (gs_check_witness_statement); the statement holds iff
        all are true"""
        m, n, arrays = self._witness_arrays(xvars, yvars)
        target = np.concatenate([np.asarray(e.target, dtype=np.uint64).reshape(-1) for e in self.equations])
        ok = crs.engine.check_witness_statement(self.TYPE, len(self.equations), m, n, *arrays, target)
        return [bool(v) for v in ok]

    def verify(self, com_proof, crs):
        """[bool per equation]; the statement holds iff all are true"""
        m, n, arrays = self._arrays(com_proof)
        ok = crs.engine.verify_statement(self.TYPE, len(self.equations), m, n, *arrays)
        return [bool(v) for v in ok]

    def _arrays(self, com_proof):
        """(m, n, the eight arrays of gs_verify_statement) after the length checks of verify()"""
        kx, ky = self._kxky()
        E = len(self.equations)
        assert len(com_proof.equ_proofs) == E
        m, n = len(com_proof.xcoms.coms), len(com_proof.ycoms.coms)
        assert m >= 1 and n >= 1
        for equ, pf in zip(self.equations, com_proof.equ_proofs):
            equ._check_statement_shape(m, n)
            assert pf.equ_type == self.TYPE and len(pf.pi) == kx and len(pf.theta) == ky
        cat = np.concatenate
        return m, n, (
            cat([_cat(e.a_consts, 0) for e in self.equations]),
            cat([_cat(e.b_consts, 0) for e in self.equations]), cat([_flat_mat(e.gamma) for e in self.equations]),
            cat([np.asarray(e.target, dtype=np.uint64).reshape(-1) for e in self.equations]),
            _cat(com_proof.xcoms.coms, 0), _cat(com_proof.ycoms.coms, 0),
            cat([_cat(pf.pi, 0) for pf in com_proof.equ_proofs]), cat([_cat(pf.theta, 0) for pf in com_proof.equ_proofs]))

    def verify_rlc(self, com_proof, crs, rng):
        """ONE verdict for the whole statement from one combined pairing check (gs_verify_statements_rlc, S = 1): the
        pairing work does not grow with the number of equations.  Accepts what verify() accepts on every equation;
        a statement with a false equation passes with probability 2^-64 over rho, which is drawn here from `rng`."""
        m, n, arrays = self._arrays(com_proof)
        E = len(self.equations)
        ok, _ = crs.engine.verify_statements_rlc(self.TYPE, 1, E, m, n, *arrays, _draw_rho(rng, 4 * E))
        return bool(ok[0])


class MixedProof:
    """Commitments of the four variable groups of a mixed-type Statement and one EquProof per equation."""

    def __init__(self, com_xg, com_yg, com_xs, com_ys, equ_proofs):
        self.com_xg, self.com_yg, self.com_xs, self.com_ys, self.equ_proofs = com_xg, com_yg, com_xs, com_ys, equ_proofs


class MixedStatement:
    """`Statement = Vec<dyn Equ>` (statement.rs:24-28,109) with equations of ANY type over one list of variables:
    G1 variables xg, G2 variables yg and scalar variables xs (committed into B1), ys (into B2).  A PPE is over
    (xg, yg), an MSMEG1 over (xg, ys), an MSMEG2 over (xs, yg), a QuadEqu over (xs, ys)  (statement.rs:117-192: which
    side of each type is a group element).  Every group is committed ONCE (batch_commit_G1 / _G2 / _scalar_to_B1 /
    _scalar_to_B2), every equation gets its own EquProof against those commitments -- what the reference does when
    one calls `equ.prove(..)` per equation with shared Commit1 / Commit2 -- and all equations of all types go to the
    engine in ONE call (gs_prove_mixed / gs_verify_mixed with shared_vars parts).  RNG draw order: the four commit
    randomness matrices (xg, yg, xs, ys), then T of equation 0, 1, ..."""

    def __init__(self, equations):
        assert len(equations) >= 1
        self.equations = list(equations)

    @staticmethod
    def _groups(ty):
        return ("xg" if ty in (GS_PPE, GS_MSMEG1) else "xs"), ("yg" if ty in (GS_PPE, GS_MSMEG2) else "ys")

    def _by_type(self):
        order = []
        for e in self.equations:
            if e.TYPE not in order:
                order.append(e.TYPE)
        return [(ty, [i for i, e in enumerate(self.equations) if e.TYPE == ty]) for ty in order]

    def commit_and_prove(self, xg, yg, xs, ys, crs, rng):
        vars_ = dict(xg=xg, yg=yg, xs=xs, ys=ys)
        coms = dict(xg=batch_commit_G1(xg, crs, rng), yg=batch_commit_G2(yg, crs, rng),
                    xs=batch_commit_scalar_to_B1(xs, crs, rng), ys=batch_commit_scalar_to_B2(ys, crs, rng))
        Ts = []
        for e in self.equations:
            kx, ky = e._kxky()
            Ts.append([[rng.fr() for _ in range(kx)] for _ in range(ky)])
        cat = np.concatenate
        parts = []
        for ty, idx in self._by_type():
            gx, gy = self._groups(ty)
            m, n = len(vars_[gx]), len(vars_[gy])
            assert m >= 1 and n >= 1
            eqs = [self.equations[i] for i in idx]
            for e in eqs:
                e._check_statement_shape(m, n)
            parts.append(dict(ty=ty, N=len(idx), m=m, n=n, shared=True, want_coms=False, X=_cat(vars_[gx], 0),
                              Y=_cat(vars_[gy], 0), A=cat([_cat(e.a_consts, 0) for e in eqs]),
                              B=cat([_cat(e.b_consts, 0) for e in eqs]), Gamma=cat([_flat_mat(e.gamma) for e in eqs]),
                              R=_flat_mat(coms[gx].rand), S=_flat_mat(coms[gy].rand),
                              T=cat([_flat_mat(Ts[i]) for i in idx])))
        outs = crs.engine.prove_mixed(parts)
        proofs = [None] * len(self.equations)
        for (ty, idx), o in zip(self._by_type(), outs):
            kx, ky = self.equations[idx[0]]._kxky()
            pis, ths = _split(o["pi"], len(idx) * kx), _split(o["theta"], len(idx) * ky)
            for k, i in enumerate(idx):
                proofs[i] = EquProof(pis[k * kx:(k + 1) * kx], ths[k * ky:(k + 1) * ky], ty, Ts[i])
        return MixedProof(coms["xg"], coms["yg"], coms["xs"], coms["ys"], proofs)

    def verify(self, proof, crs):
        """[bool per equation], in the order of the statement's equations"""
        oks = crs.engine.verify_mixed(self._verify_parts(proof))
        out = [None] * len(self.equations)
        for (ty, idx), ok in zip(self._by_type(), oks):
            for k, i in enumerate(idx):
                out[i] = bool(ok[k])
        return out

    def verify_rlc(self, proof, crs, rng):
        """ONE verdict for the whole mixed statement: one combined check per equation type
        (gs_verify_statements_rlc, S = 1) and one gs_gt_finalize over the types' accumulator pairs."""
        pairs = []
        for p in self._verify_parts(proof):
            _, acc = crs.engine.verify_statements_rlc(p["ty"], 1, p["N"], p["m"], p["n"], p["A"], p["B"], p["Gamma"],
                                                      p["target"], p["xcoms"], p["ycoms"], p["pi"], p["theta"],
                                                      _draw_rho(rng, 4 * p["N"]))
            pairs.append(acc.reshape(-1))
        return bool(crs.engine.gt_finalize(np.concatenate(pairs)))

    def _verify_parts(self, proof):
        """one shared-variables part per equation type, in the order of _by_type()"""
        coms = dict(xg=proof.com_xg, yg=proof.com_yg, xs=proof.com_xs, ys=proof.com_ys)
        assert len(proof.equ_proofs) == len(self.equations)
        cat = np.concatenate
        parts = []
        for ty, idx in self._by_type():
            gx, gy = self._groups(ty)
            m, n = len(coms[gx].coms), len(coms[gy].coms)
            assert m >= 1 and n >= 1
            eqs = [self.equations[i] for i in idx]
            pfs = [proof.equ_proofs[i] for i in idx]
            kx, ky = eqs[0]._kxky()
            for e, pf in zip(eqs, pfs):
                e._check_statement_shape(m, n)
                assert pf.equ_type == ty and len(pf.pi) == kx and len(pf.theta) == ky
            parts.append(dict(ty=ty, N=len(idx), m=m, n=n, shared=True, A=cat([_cat(e.a_consts, 0) for e in eqs]),
                              B=cat([_cat(e.b_consts, 0) for e in eqs]), Gamma=cat([_flat_mat(e.gamma) for e in eqs]),
                              target=cat([np.asarray(e.target, dtype=np.uint64).reshape(-1) for e in eqs]),
                              xcoms=_cat(coms[gx].coms, 0), ycoms=_cat(coms[gy].coms, 0),
                              pi=cat([_cat(pf.pi, 0) for pf in pfs]), theta=cat([_cat(pf.theta, 0) for pf in pfs])))
        return parts
