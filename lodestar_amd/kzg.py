"""KZG commitments for EIP-4844 blobs on the GPU.

Mirrors the c-kzg surface Lodestar binds in packages/beacon-node/src/util/kzg.ts:15-65
(`loadTrustedSetup`, `blobToKzgCommitment`, `computeAggregateKzgProof`, `verifyAggregateKzgProof`;
callers chain/validation/blobsSidecar.ts:75-120 and chain/produceBlock/validateBlobsAndKzgCommitments.ts)
following the EIP-4844 polynomial-commitments spec of the reference's pinned consensus-spec
version (v1.3.0-alpha.2, test/spec/specTestVersioning.ts:18).

Split, chosen per `Kzg(engine, field=...)`:

* field="host" (the default): the scalar-field work is host code here (the inverse FFT from the
  blob's evaluations to monomial coefficients, Fiat-Shamir challenges, evaluation, quotient); the
  group work runs on the GPU through the C ABI -- 4096-term G1 linear combinations of the resident
  trusted setup (`lb_g1_lincomb`) and the proof check as one two-pair pairing product
  (`lb_kzg_verify_proof`).
* field="device": the blob-level C calls (`lb_kzg_blob_to_commitment`,
  `lb_kzg_compute_aggregate_proof`, `lb_kzg_verify_aggregate_proof`, `lb_kzg_compute_proof`,
  `lb_kzg_blob_coefficients`) take the blobs' bytes; the field work runs in the k_fr_* kernels
  (csrc/lb_kzg_field.h), only the transcript hash stays on the host (in C).  Same bytes out.

Whatever `field` is, `verify_aggregate_kzg_proof_batch` checks many sidecars (a range-sync segment's
blocks) in one pass over the GPU (`lb_kzg_verify_aggregate_proof_batch`), one verdict per sidecar.

The per-blob proof form that shipped in Deneb (c-kzg `computeBlobKzgProof`, `verifyBlobKzgProof`,
`verifyBlobKzgProofBatch`, `computeKzgProof`, `verifyKzgProof`) is here too: `compute_challenge` and
`compute_batch_r` restate its two transcripts, `Kzg.compute_blob_kzg_proof` and
`Kzg.verify_blob_kzg_proof` honour `field` (same bytes either way), and the batch calls
(`verify_blob_kzg_proof_batch`, `verify_blob_kzg_proof_batch_many` for many blocks' sidecars in one
pass) always run on the GPU (`lb_kzg_verify_blob_proof_batch`).

Cells (EIP-7594, "PeerDAS", the Fulu fork; c-kzg `computeCells`, `verifyCellKzgProofBatch`): the
blob's polynomial over the 8192-point domain in 128 cells of 64 values, each cell with its own proof.
`Kzg.compute_cells`, `Kzg.compute_cell_kzg_proofs` (the direct per-cell route, one multi-scalar
multiplication per cell), `Kzg.compute_cells_and_kzg_proofs(_many)` (c-kzg `computeCellsAndKzgProofs`:
all 128 proofs of a blob by FK20), `Kzg.recover_cells_and_kzg_proofs(_many)` (c-kzg
`recoverCellsAndKzgProofs`: all cells and proofs of a blob from any 64 of its cells) and
`Kzg.verify_cell_kzg_proof_batch(_many)` always run on the GPU (`lb_kzg_compute_cells`,
`lb_kzg_compute_cell_proofs`, `lb_kzg_compute_cells_and_proofs`, `lb_kzg_recover_cells_and_proofs`,
`lb_kzg_verify_cell_proof_batch`), whatever `field` is.
`compute_cell_batch_r` restates the batch's combiner; like the other transcripts its byte parity
with c-kzg is UNPINNED, and the verdicts do not depend on its exact bytes: a valid batch passes for
any r, an invalid one fails except with negligible probability.

The setup is Lodestar's own `trusted_setup.bin` (kzg.ts:36-48: two u32 counts, 4096 compressed
[tau^i] G1, 65 compressed [tau^i] G2), i.e. MONOMIAL form (setup_G1[0] is the G1 generator).
Committing in monomial form, sum a_j [tau^j] G1 with a = IFFT of the blob's evaluations, gives
exactly the spec's g1_lincomb(bit_reversal_permutation(KZG_SETUP_LAGRANGE), blob).

Parity: c-kzg is an un-vendored npm dependency with no fixtures in the reference (kzg.test.ts only
checks that its own proofs verify), so byte parity with c-kzg is UNPINNED.  Field elements are
read big-endian, as Lodestar's own range check reads them (blobsSidecar.ts:138-150); the
transcript follows the spec's compute_challenges with the same byte order.  Tests pin the
mathematics against the independent oracle restatement (oracle/kzg.py).
"""
from __future__ import annotations

import ctypes
import hashlib
import os
from typing import List, Sequence, Tuple

import numpy as np

BLS_MODULUS = 52435875175126190479447740508185965837690552500527637822603658699938581184513
FIELD_ELEMENTS_PER_BLOB = 4096
BYTES_PER_FIELD_ELEMENT = 32
BYTES_PER_BLOB = FIELD_ELEMENTS_PER_BLOB * BYTES_PER_FIELD_ELEMENT
FIAT_SHAMIR_PROTOCOL_DOMAIN = b"FSBLOBVERIFY_V1_"
PRIMITIVE_ROOT_OF_UNITY = 7
ENDIANNESS = "big"
TRUSTED_SETUP_BIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "trusted_setup.bin")

G1_COUNT, G1_BYTES, G2_COUNT, G2_BYTES = FIELD_ELEMENTS_PER_BLOB, 48, 65, 96


def read_trusted_setup_bin(data: bytes) -> Tuple[List[bytes], List[bytes]]:
    """kzg.ts trustedSetupBinToJson: skip the two u32 counts, then 4096 x 48 B G1, 65 x 96 B G2."""
    total = 8 + G1_COUNT * G1_BYTES + G2_COUNT * G2_BYTES
    if len(data) < total:
        raise ValueError(f"trusted_setup size {len(data)} < {total}")
    g1 = [bytes(data[8 + i * 48: 8 + (i + 1) * 48]) for i in range(G1_COUNT)]
    base = 8 + G1_COUNT * G1_BYTES
    g2 = [bytes(data[base + i * 96: base + (i + 1) * 96]) for i in range(G2_COUNT)]
    return g1, g2


# ------------------------------------------------------------------ scalar field (host)
def _roots_of_unity(n: int) -> List[int]:
    w = pow(PRIMITIVE_ROOT_OF_UNITY, (BLS_MODULUS - 1) // n, BLS_MODULUS)
    out, x = [], 1
    for _ in range(n):
        out.append(x)
        x = x * w % BLS_MODULUS
    return out


def _brp_index(n: int) -> List[int]:
    bits = n.bit_length() - 1
    return [int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)]


ROOTS = _roots_of_unity(FIELD_ELEMENTS_PER_BLOB)
BRP = _brp_index(FIELD_ELEMENTS_PER_BLOB)
ROOTS_BRP = [ROOTS[BRP[i]] for i in range(FIELD_ELEMENTS_PER_BLOB)]


def _ntt(a: List[int], roots: List[int]) -> List[int]:
    """in-order radix-2 transform: out[k] = sum_j a[j] roots[j k mod n]"""
    n = len(a)
    idx = BRP if n == FIELD_ELEMENTS_PER_BLOB else _brp_index(n)
    a = [a[idx[i]] for i in range(n)]
    m = 1
    while m < n:
        step = n // (2 * m)
        for s in range(0, n, 2 * m):
            for j in range(m):
                w = roots[j * step]
                u, v = a[s + j], a[s + j + m] * w % BLS_MODULUS
                a[s + j] = (u + v) % BLS_MODULUS
                a[s + j + m] = (u - v) % BLS_MODULUS
        m *= 2
    return a


def blob_to_polynomial(blob: bytes) -> List[int]:
    """the blob's 4096 field elements (its evaluations at the bit-reversed roots of unity)"""
    if len(blob) != BYTES_PER_BLOB:
        raise ValueError(f"blob length {len(blob)} != {BYTES_PER_BLOB}")
    out = []
    for i in range(FIELD_ELEMENTS_PER_BLOB):
        v = int.from_bytes(blob[32 * i: 32 * i + 32], ENDIANNESS)
        if v >= BLS_MODULUS:
            raise ValueError("blob field element >= BLS_MODULUS")
        out.append(v)
    return out


def evaluations_to_coefficients(poly: Sequence[int]) -> List[int]:
    """monomial coefficients of the polynomial with p(ROOTS_BRP[i]) = poly[i] (inverse NTT)"""
    n = len(poly)
    nat = [0] * n
    for i, v in enumerate(poly):
        nat[BRP[i]] = v
    inv_roots = [ROOTS[(-k) % n] for k in range(n)]
    inv_n = pow(n, BLS_MODULUS - 2, BLS_MODULUS)
    return [c * inv_n % BLS_MODULUS for c in _ntt(nat, inv_roots)]


def evaluate_coefficients(coeffs: Sequence[int], z: int) -> int:
    y = 0
    for c in reversed(coeffs):
        y = (y * z + c) % BLS_MODULUS
    return y


def quotient_coefficients(coeffs: Sequence[int], z: int) -> List[int]:
    """(p(X) - p(z)) / (X - z) by synthetic division"""
    n = len(coeffs)
    q = [0] * (n - 1)
    acc = 0
    for k in range(n - 1, 0, -1):
        acc = (acc * z + coeffs[k]) % BLS_MODULUS
        q[k - 1] = acc
    return q


def hash_to_bls_field(data: bytes) -> int:
    return int.from_bytes(hashlib.sha256(data).digest(), ENDIANNESS) % BLS_MODULUS


def compute_challenges(polys: Sequence[Sequence[int]], commitments: Sequence[bytes]) -> Tuple[List[int], int]:
    """spec compute_challenges: transcript = domain || degree (8 B) || count (8 B) || every field
    element (32 B) || every commitment (48 B); r = H(h || 0x00), x = H(h || 0x01)"""
    data = bytearray(FIAT_SHAMIR_PROTOCOL_DOMAIN)
    data += FIELD_ELEMENTS_PER_BLOB.to_bytes(8, ENDIANNESS)
    data += len(polys).to_bytes(8, ENDIANNESS)
    for p in polys:
        for v in p:
            data += int(v).to_bytes(BYTES_PER_FIELD_ELEMENT, ENDIANNESS)
    for c in commitments:
        data += bytes(c)
    h = hashlib.sha256(bytes(data)).digest()
    r = hash_to_bls_field(h + b"\x00")
    powers, x = [], 1
    for _ in range(len(commitments)):
        powers.append(x)
        x = x * r % BLS_MODULUS
    return powers, hash_to_bls_field(h + b"\x01")


# -- one proof per blob (Deneb): each blob has its own transcript, and a batch its own combiner
RANDOM_CHALLENGE_KZG_BATCH_DOMAIN = b"RCKZGBATCH___V1_"


def compute_challenge(blob: bytes, commitment: bytes) -> int:
    """z = hash_to_bls_field(domain || 4096 as 16 bytes || blob || commitment); no tag byte"""
    if len(blob) != BYTES_PER_BLOB or len(commitment) != 48:
        raise ValueError("compute_challenge: a 131072-byte blob and a 48-byte commitment")
    return hash_to_bls_field(FIAT_SHAMIR_PROTOCOL_DOMAIN + FIELD_ELEMENTS_PER_BLOB.to_bytes(16, ENDIANNESS)
                             + bytes(blob) + bytes(commitment))


def compute_batch_r(commitments: Sequence[bytes], zs: Sequence[int], ys: Sequence[int], proofs: Sequence[bytes]) -> int:
    """the combiner of verify_blob_kzg_proof_batch: domain || 4096 and n as 8 bytes each || per blob
    commitment (48) || z (32) || y (32) || proof (48)"""
    n = len(commitments)
    if not (len(zs) == len(ys) == len(proofs) == n):
        raise ValueError("compute_batch_r: one z, y and proof per commitment")
    data = bytearray(RANDOM_CHALLENGE_KZG_BATCH_DOMAIN)
    data += FIELD_ELEMENTS_PER_BLOB.to_bytes(8, ENDIANNESS) + n.to_bytes(8, ENDIANNESS)
    for c, z, y, p in zip(commitments, zs, ys, proofs):
        data += bytes(c) + int(z).to_bytes(32, ENDIANNESS) + int(y).to_bytes(32, ENDIANNESS) + bytes(p)
    return hash_to_bls_field(bytes(data))


# -- cells (EIP-7594): the extended domain, the cosets, the batch combiner
FIELD_ELEMENTS_PER_EXT_BLOB = 8192
FIELD_ELEMENTS_PER_CELL = 64
BYTES_PER_CELL = FIELD_ELEMENTS_PER_CELL * BYTES_PER_FIELD_ELEMENT
CELLS_PER_EXT_BLOB = FIELD_ELEMENTS_PER_EXT_BLOB // FIELD_ELEMENTS_PER_CELL
MAX_BLOBS_PER_CELLS_AND_PROOFS_CALL = 128   # lb_kzg_compute_cells_and_proofs' limit; longer lists go in passes
RANDOM_CHALLENGE_KZG_CELL_BATCH_DOMAIN = b"RCKZGCBATCH__V1_"
ROOT_OF_UNITY_EXT = pow(PRIMITIVE_ROOT_OF_UNITY, (BLS_MODULUS - 1) // FIELD_ELEMENTS_PER_EXT_BLOB, BLS_MODULUS)


def coset_shift(cell_index: int) -> int:
    """h_i = w^brp7(i): element t of cell i stands at h_i * w64^brp6(t), w64 = w^128"""
    if not 0 <= cell_index < CELLS_PER_EXT_BLOB:
        raise ValueError(f"cell index {cell_index} not below {CELLS_PER_EXT_BLOB}")
    return pow(ROOT_OF_UNITY_EXT, int(format(cell_index, "07b")[::-1], 2), BLS_MODULUS)


def compute_cell_batch_r(commitments: Sequence[bytes], cell_indices: Sequence[int], cells: Sequence[bytes],
                         proofs: Sequence[bytes]) -> int:
    """the combiner of verify_cell_kzg_proof_batch over one commitment, cell index, cell and proof per
    cell: the commitments deduplicated in order of first appearance, then domain || 4096 || 64 ||
    #distinct || n || the distinct commitments || per cell: commitment index || cell index || cell
    (2048) || proof (48); every integer 8 bytes big-endian"""
    n = len(cells)
    if not (len(commitments) == len(cell_indices) == len(proofs) == n):
        raise ValueError("compute_cell_batch_r: one commitment, cell index and proof per cell")
    distinct, index_of = [], {}
    for c in commitments:
        if bytes(c) not in index_of:
            index_of[bytes(c)] = len(distinct)
            distinct.append(bytes(c))
    data = bytearray(RANDOM_CHALLENGE_KZG_CELL_BATCH_DOMAIN)
    for v in (FIELD_ELEMENTS_PER_BLOB, FIELD_ELEMENTS_PER_CELL, len(distinct), n):
        data += v.to_bytes(8, ENDIANNESS)
    data += b"".join(distinct)
    for c, i, cell, p in zip(commitments, cell_indices, cells, proofs):
        data += index_of[bytes(c)].to_bytes(8, ENDIANNESS) + int(i).to_bytes(8, ENDIANNESS) + bytes(cell) + bytes(p)
    return hash_to_bls_field(bytes(data))


def _scalars_le(vals: Sequence[int]) -> np.ndarray:
    out = np.zeros((len(vals), 32), np.uint8)
    for i, v in enumerate(vals):
        out[i] = np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)
    return out


# ------------------------------------------------------------------ GPU-backed KZG
G1_INFINITY48 = b"\xc0" + b"\x00" * 47  # compressed point at infinity


class KzgError(Exception):
    pass


class Kzg:
    """ckzg for one engine: `load_trusted_setup` once, then commitments / aggregate proofs."""

    def __init__(self, engine, setup: bytes = None, field: str = "host"):
        from lodestar_amd import _native as N
        if field not in ("host", "device"):
            raise ValueError('field must be "host" or "device"')
        self.field = field
        self.engine = engine
        self.lib = N.load()
        self._N = N
        if setup is None:
            with open(TRUSTED_SETUP_BIN, "rb") as f:
                setup = f.read()
        self.load_trusted_setup(setup)

    def _check(self, st: int, what: str):
        if st != 0:
            raise KzgError(f"{what}: {self._N.error_name(st)}")

    def load_trusted_setup(self, setup_bin: bytes) -> None:
        g1, g2 = read_trusted_setup_bin(setup_bin)
        g1b = np.frombuffer(b"".join(g1), np.uint8)
        g2b = np.frombuffer(b"".join(g2), np.uint8)
        status = np.zeros(len(g1), np.int32)
        u8 = ctypes.POINTER(ctypes.c_uint8)
        st = self.lib.lb_kzg_load_setup(self.engine.h, g1b.ctypes.data_as(u8), len(g1), g2b.ctypes.data_as(u8),
                                        len(g2), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        self._check(st, "loadTrustedSetup")

    def g1_lincomb(self, scalars: Sequence[int], points48: Sequence[bytes] = None) -> bytes:
        """sum s_i P_i with P_i the setup's [tau^i] G1 (points48 None) or the given points"""
        n = len(scalars)
        sc = _scalars_le(scalars)
        out = (ctypes.c_uint8 * 48)()
        u8 = ctypes.POINTER(ctypes.c_uint8)
        pts = None
        if points48 is not None:
            if len(points48) != n or any(len(p) != 48 for p in points48):
                raise KzgError("g1_lincomb: points must be 48-byte compressed, one per scalar")
            pts = np.frombuffer(b"".join(bytes(p) for p in points48), np.uint8)
        st = self.lib.lb_g1_lincomb(self.engine.h, n, None if pts is None else pts.ctypes.data_as(u8),
                                    sc.ctypes.data_as(u8), ctypes.cast(out, u8))
        self._check(st, "g1_lincomb")
        return bytes(out)

    def commit_coefficients(self, coeffs: Sequence[int]) -> bytes:
        return self.g1_lincomb(coeffs)

    # -- field="device": bytes straight to the blob-level C calls
    @staticmethod
    def _blob_bytes(blobs: Sequence[bytes]) -> np.ndarray:
        for b in blobs:
            if len(b) != BYTES_PER_BLOB:
                raise ValueError(f"blob length {len(b)} != {BYTES_PER_BLOB}")
        return np.frombuffer(b"".join(bytes(b) for b in blobs) or b"\x00", np.uint8)

    def blob_coefficients(self, blob: bytes) -> List[int]:
        """monomial coefficients of the blob's polynomial, computed on the GPU (`lb_kzg_blob_coefficients`)"""
        u8 = ctypes.POINTER(ctypes.c_uint8)
        src = self._blob_bytes([blob])
        out = np.zeros(BYTES_PER_BLOB, np.uint8)
        self._check(self.lib.lb_kzg_blob_coefficients(self.engine.h, src.ctypes.data_as(u8), out.ctypes.data_as(u8)),
                    "blob_coefficients")
        raw = out.tobytes()
        return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(FIELD_ELEMENTS_PER_BLOB)]

    def compute_kzg_proof(self, blob: bytes, z: int) -> Tuple[bytes, int]:
        """(proof, y): the proof that the blob's polynomial takes the value y at z, on the GPU
        (`lb_kzg_compute_proof`); z may lie on the evaluation domain"""
        u8 = ctypes.POINTER(ctypes.c_uint8)
        src = self._blob_bytes([blob])
        zb = (ctypes.c_uint8 * 32).from_buffer_copy(int(z).to_bytes(32, "little"))
        proof = (ctypes.c_uint8 * 48)()
        yb = (ctypes.c_uint8 * 32)()
        self._check(self.lib.lb_kzg_compute_proof(self.engine.h, src.ctypes.data_as(u8), ctypes.cast(zb, u8),
                                                  ctypes.cast(proof, u8), ctypes.cast(yb, u8)), "compute_kzg_proof")
        return bytes(proof), int.from_bytes(bytes(yb), "little")

    def _device_commitments(self, blobs: Sequence[bytes]) -> List[bytes]:
        u8 = ctypes.POINTER(ctypes.c_uint8)
        n = len(blobs)
        src = self._blob_bytes(blobs)
        out = np.zeros(48 * max(n, 1), np.uint8)
        status = np.zeros(max(n, 1), np.int32)
        self._check(self.lib.lb_kzg_blob_to_commitment(self.engine.h, n, src.ctypes.data_as(u8), out.ctypes.data_as(u8),
                                                       status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
                    "blobToKzgCommitment")
        for b in range(n):
            self._check(int(status[b]), f"blobToKzgCommitment: blob {b}")
        return [out[48 * b: 48 * b + 48].tobytes() for b in range(n)]

    def blob_to_kzg_commitment(self, blob: bytes) -> bytes:
        if self.field == "device":
            return self._device_commitments([blob])[0]
        return self.commit_coefficients(evaluations_to_coefficients(blob_to_polynomial(blob)))

    def _aggregate(self, blobs: Sequence[bytes], commitments: Sequence[bytes]):
        polys = [blob_to_polynomial(b) for b in blobs]
        r_powers, x = compute_challenges(polys, commitments)
        agg = [sum(r_powers[j] * polys[j][i] for j in range(len(polys))) % BLS_MODULUS
               for i in range(FIELD_ELEMENTS_PER_BLOB)]
        return agg, r_powers, x

    def compute_kzg_proof_coefficients(self, coeffs: Sequence[int], z: int) -> Tuple[bytes, int]:
        return self.commit_coefficients(quotient_coefficients(coeffs, z)), evaluate_coefficients(coeffs, z)

    def compute_aggregate_kzg_proof(self, blobs: Sequence[bytes]) -> bytes:
        """c-kzg compute_aggregate_kzg_proof; called for every produced block (chain.ts:402), blobless
        ones included: zero blobs aggregate to the zero polynomial, whose proof is the point at
        infinity (the spec's compute_kzg_proof of the zero polynomial)."""
        if self.field == "device":
            u8 = ctypes.POINTER(ctypes.c_uint8)
            src = self._blob_bytes(blobs)
            out = (ctypes.c_uint8 * 48)()
            self._check(self.lib.lb_kzg_compute_aggregate_proof(self.engine.h, len(blobs), src.ctypes.data_as(u8),
                                                                ctypes.cast(out, u8)), "computeAggregateKzgProof")
            return bytes(out)
        if not blobs:
            return G1_INFINITY48
        commitments = [self.blob_to_kzg_commitment(b) for b in blobs]
        agg, _, x = self._aggregate(blobs, commitments)
        proof, _ = self.compute_kzg_proof_coefficients(evaluations_to_coefficients(agg), x)
        return proof

    def verify_kzg_proof(self, commitment: bytes, z: int, y: int, proof: bytes) -> bool:
        if len(commitment) != 48 or len(proof) != 48:
            raise KzgError("verify_kzg_proof: 48-byte commitment and proof")
        ok = ctypes.c_int32(0)
        u8 = ctypes.POINTER(ctypes.c_uint8)
        zb = (ctypes.c_uint8 * 32).from_buffer_copy(int(z).to_bytes(32, "little"))
        yb = (ctypes.c_uint8 * 32).from_buffer_copy(int(y).to_bytes(32, "little"))
        cb = (ctypes.c_uint8 * 48).from_buffer_copy(bytes(commitment))
        pb = (ctypes.c_uint8 * 48).from_buffer_copy(bytes(proof))
        st = self.lib.lb_kzg_verify_proof(self.engine.h, ctypes.cast(cb, u8), ctypes.cast(zb, u8),
                                          ctypes.cast(yb, u8), ctypes.cast(pb, u8), ctypes.byref(ok))
        self._check(st, "verify_kzg_proof")
        if ok.value < 0:
            raise KzgError(f"verify_kzg_proof: {self._N.error_name(-ok.value)}")
        return ok.value == 1

    def verify_aggregate_kzg_proof(self, blobs: Sequence[bytes], commitments: Sequence[bytes], proof: bytes) -> bool:
        if len(blobs) != len(commitments):
            raise KzgError("verifyAggregateKzgProof: blobs / commitments length mismatch")
        if self.field == "device":
            if len(proof) != 48 or any(len(c) != 48 for c in commitments):
                raise KzgError("verifyAggregateKzgProof: 48-byte commitments and proof")
            u8 = ctypes.POINTER(ctypes.c_uint8)
            src = self._blob_bytes(blobs)
            cm = np.frombuffer(b"".join(bytes(c) for c in commitments) or b"\x00", np.uint8)
            pb = (ctypes.c_uint8 * 48).from_buffer_copy(bytes(proof))
            ok = ctypes.c_int32(0)
            self._check(self.lib.lb_kzg_verify_aggregate_proof(self.engine.h, len(blobs), src.ctypes.data_as(u8),
                                                               cm.ctypes.data_as(u8), ctypes.cast(pb, u8),
                                                               ctypes.byref(ok)), "verifyAggregateKzgProof")
            if ok.value < 0:
                raise KzgError(f"verifyAggregateKzgProof: {self._N.error_name(-ok.value)}")
            return ok.value == 1
        if not blobs:
            # aggregated commitment = infinity, y = 0: e(pi, [tau - z] G2) == 1 iff pi is infinity
            # (the check still decodes pi: a malformed proof raises)
            return self.verify_kzg_proof(G1_INFINITY48, compute_challenges([], [])[1], 0, proof)
        agg, r_powers, x = self._aggregate(blobs, commitments)
        c = self.g1_lincomb(r_powers, list(commitments))
        y = evaluate_coefficients(evaluations_to_coefficients(agg), x)
        return self.verify_kzg_proof(c, x, y, proof)

    def verify_aggregate_kzg_proof_batch(self, sidecars: Sequence[Tuple[Sequence[bytes], Sequence[bytes], bytes]]) -> list:
        """verify_aggregate_kzg_proof for many sidecars (a range-sync segment's blocks) in one pass
        over the GPU (`lb_kzg_verify_aggregate_proof_batch`), whatever `field` is.  `sidecars`:
        (blobs, commitments, proof) each.  One entry per sidecar: True, False, or the KzgError the
        single call would raise -- returned, not raised, so one bad sidecar does not hide the others.
        Malformed input (a blobs / commitments length mismatch, a wrong blob or point length) raises
        before anything is sent."""
        what = "verifyAggregateKzgProof"
        offsets, blobs, comms, proofs = [0], [], [], []
        for sc_blobs, sc_comms, proof in sidecars:
            if len(sc_blobs) != len(sc_comms):
                raise KzgError(f"{what}: blobs / commitments length mismatch")
            if len(proof) != 48 or any(len(c) != 48 for c in sc_comms):
                raise KzgError(f"{what}: 48-byte commitments and proof")
            blobs += list(sc_blobs)
            comms += [bytes(c) for c in sc_comms]
            proofs.append(bytes(proof))
            offsets.append(len(blobs))
        n = len(proofs)
        if n == 0:
            return []
        u8, i32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
        src = self._blob_bytes(blobs)
        cm = np.frombuffer(b"".join(comms) or b"\x00", np.uint8)
        pf = np.frombuffer(b"".join(proofs), np.uint8)
        off = np.asarray(offsets, np.uint32)
        ok = np.zeros(n, np.int32)
        self._check(self.lib.lb_kzg_verify_aggregate_proof_batch(
            self.engine.h, n, off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), src.ctypes.data_as(u8),
            cm.ctypes.data_as(u8), pf.ctypes.data_as(u8), ok.ctypes.data_as(i32)), f"{what}Batch")
        return [KzgError(f"{what}: {self._N.error_name(-int(v))}") if v < 0 else bool(v == 1) for v in ok]

    # -- one proof per blob (Deneb): computeBlobKzgProof, verifyBlobKzgProof(Batch), computeKzgProof, verifyKzgProof
    @staticmethod
    def _points48(what: str, *groups: Sequence[bytes]) -> None:
        if any(len(p) != 48 for g in groups for p in g):
            raise KzgError(f"{what}: 48-byte commitments and proofs")

    def compute_blob_kzg_proof(self, blob: bytes, commitment: bytes) -> bytes:
        """the proof that the blob's polynomial takes the value p(z) at z = compute_challenge(blob,
        commitment); the commitment must decode and lie in G1 (infinity allowed)"""
        what = "computeBlobKzgProof"
        self._points48(what, [commitment])
        if self.field == "device":
            u8, i32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
            src = self._blob_bytes([blob])
            cm = np.frombuffer(bytes(commitment), np.uint8)
            out = np.zeros(48, np.uint8)
            status = np.zeros(1, np.int32)
            self._check(self.lib.lb_kzg_compute_blob_proofs(self.engine.h, 1, src.ctypes.data_as(u8), cm.ctypes.data_as(u8),
                                                            out.ctypes.data_as(u8), status.ctypes.data_as(i32)), what)
            self._check(int(status[0]), what)
            return out.tobytes()
        self.g1_lincomb([1], [commitment])  # decodes and subgroup-checks the commitment
        coeffs = evaluations_to_coefficients(blob_to_polynomial(blob))
        return self.commit_coefficients(quotient_coefficients(coeffs, compute_challenge(blob, commitment)))

    def verify_blob_kzg_proof_batch_many(self, groups: Sequence[Tuple[Sequence[bytes], Sequence[bytes], Sequence[bytes]]]) -> list:
        """verify_blob_kzg_proof_batch for many groups (one group = one block's sidecars: blobs,
        commitments, proofs, one proof per blob) in one pass over the GPU
        (`lb_kzg_verify_blob_proof_batch`), whatever `field` is.  One entry per group: True, False,
        or the KzgError the single call would raise -- returned, not raised.  Malformed input (length
        mismatches, a wrong blob or point length) raises before anything is sent."""
        what = "verifyBlobKzgProofBatch"
        offsets, blobs, comms, proofs = [0], [], [], []
        for g_blobs, g_comms, g_proofs in groups:
            if not (len(g_blobs) == len(g_comms) == len(g_proofs)):
                raise KzgError(f"{what}: blobs / commitments / proofs length mismatch")
            self._points48(what, g_comms, g_proofs)
            blobs += list(g_blobs)
            comms += [bytes(c) for c in g_comms]
            proofs += [bytes(p) for p in g_proofs]
            offsets.append(len(blobs))
        n = len(offsets) - 1
        if n == 0:
            return []
        u8, i32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
        src = self._blob_bytes(blobs)
        cm = np.frombuffer(b"".join(comms) or b"\x00", np.uint8)
        pf = np.frombuffer(b"".join(proofs) or b"\x00", np.uint8)
        off = np.asarray(offsets, np.uint32)
        ok = np.zeros(n, np.int32)
        self._check(self.lib.lb_kzg_verify_blob_proof_batch(
            self.engine.h, n, off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), src.ctypes.data_as(u8),
            cm.ctypes.data_as(u8), pf.ctypes.data_as(u8), ok.ctypes.data_as(i32)), f"{what}Many")
        return [KzgError(f"{what}: {self._N.error_name(-int(v))}") if v < 0 else bool(v == 1) for v in ok]

    def verify_blob_kzg_proof_batch(self, blobs: Sequence[bytes], commitments: Sequence[bytes], proofs: Sequence[bytes]) -> bool:
        """c-kzg verifyBlobKzgProofBatch: one group, always through the device call"""
        res = self.verify_blob_kzg_proof_batch_many([(blobs, commitments, proofs)])[0]
        if isinstance(res, KzgError):
            raise res
        return res

    def verify_blob_kzg_proof(self, blob: bytes, commitment: bytes, proof: bytes) -> bool:
        """c-kzg verifyBlobKzgProof: the batch of one blob (r^0 = 1)"""
        if self.field == "device":
            return self.verify_blob_kzg_proof_batch([blob], [commitment], [proof])
        self._points48("verifyBlobKzgProof", [commitment], [proof])
        self.g1_lincomb([1], [commitment])  # the commitment's error comes before the blob's
        z = compute_challenge(blob, commitment)
        y = evaluate_coefficients(evaluations_to_coefficients(blob_to_polynomial(blob)), z)
        return self.verify_kzg_proof(commitment, z, y, proof)

    @staticmethod
    def _field_element(what: str, b: bytes) -> int:
        if len(b) != 32:
            raise KzgError(f"{what}: 32-byte field elements")
        v = int.from_bytes(bytes(b), ENDIANNESS)
        if v >= BLS_MODULUS:
            raise KzgError(f"{what}: BLST_BAD_SCALAR")
        return v

    def compute_kzg_proof_bytes(self, blob: bytes, z32: bytes) -> Tuple[bytes, bytes]:
        """c-kzg computeKzgProof: (proof, y) with z and y as 32 big-endian bytes"""
        z = self._field_element("computeKzgProof", z32)
        if self.field == "device":
            proof, y = self.compute_kzg_proof(blob, z)
        else:
            proof, y = self.compute_kzg_proof_coefficients(evaluations_to_coefficients(blob_to_polynomial(blob)), z)
        return proof, y.to_bytes(32, ENDIANNESS)

    def verify_kzg_proof_bytes(self, commitment: bytes, z32: bytes, y32: bytes, proof: bytes) -> bool:
        """c-kzg verifyKzgProof: z and y as 32 big-endian bytes, each below r"""
        z = self._field_element("verifyKzgProof", z32)
        y = self._field_element("verifyKzgProof", y32)
        return self.verify_kzg_proof(commitment, z, y, proof)

    # -- cells (EIP-7594): computeCells, verifyCellKzgProofBatch; always on the device
    def compute_cells(self, blob: bytes) -> List[bytes]:
        """c-kzg computeCells: the blob's 128 cells of 2048 bytes (`lb_kzg_compute_cells`)"""
        u8, i32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
        src = self._blob_bytes([blob])
        out = np.zeros(CELLS_PER_EXT_BLOB * BYTES_PER_CELL, np.uint8)
        status = np.zeros(1, np.int32)
        self._check(self.lib.lb_kzg_compute_cells(self.engine.h, 1, src.ctypes.data_as(u8), out.ctypes.data_as(u8),
                                                  status.ctypes.data_as(i32)), "computeCells")
        self._check(int(status[0]), "computeCells")
        raw = out.tobytes()
        return [raw[BYTES_PER_CELL * i: BYTES_PER_CELL * (i + 1)] for i in range(CELLS_PER_EXT_BLOB)]

    def compute_cell_kzg_proofs(self, blob: bytes, cell_indices: Sequence[int]) -> List[bytes]:
        """the proofs of the chosen cells of one blob by the direct route (`lb_kzg_compute_cell_proofs`):
        one 4096-term multi-scalar multiplication per cell, so for a few cells; compute_cells_and_kzg_proofs
        gives all 128"""
        what = "computeCellKzgProofs"
        idx = [int(i) for i in cell_indices]
        if any(not 0 <= i < CELLS_PER_EXT_BLOB for i in idx):
            raise KzgError(f"{what}: cell indices below {CELLS_PER_EXT_BLOB}")
        u8, i32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
        src = self._blob_bytes([blob])
        ci = np.asarray(idx or [0], np.uint32)
        out = np.zeros(48 * max(len(idx), 1), np.uint8)
        status = np.zeros(1, np.int32)
        self._check(self.lib.lb_kzg_compute_cell_proofs(self.engine.h, src.ctypes.data_as(u8), len(idx),
                                                        ci.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                        out.ctypes.data_as(u8), status.ctypes.data_as(i32)), what)
        self._check(int(status[0]), what)
        return [out[48 * c: 48 * c + 48].tobytes() for c in range(len(idx))]

    def compute_cells_and_kzg_proofs_many(self, blobs: Sequence[bytes]) -> list:
        """compute_cells_and_kzg_proofs for many blobs in passes of up to 128 over the GPU
        (`lb_kzg_compute_cells_and_proofs`: FK20), whatever `field` is.  One entry per blob: the pair
        (128 cells, 128 proofs), or the KzgError the single call would raise -- returned, not raised.
        A wrong blob length raises before anything is sent."""
        what = "computeCellsAndKzgProofs"
        for b in blobs:
            if len(b) != BYTES_PER_BLOB:
                raise ValueError(f"blob length {len(b)} != {BYTES_PER_BLOB}")
        u8, i32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
        res: list = []
        for lo in range(0, len(blobs), MAX_BLOBS_PER_CELLS_AND_PROOFS_CALL):
            part = blobs[lo: lo + MAX_BLOBS_PER_CELLS_AND_PROOFS_CALL]
            n = len(part)
            src = self._blob_bytes(part)
            cells = np.zeros(n * CELLS_PER_EXT_BLOB * BYTES_PER_CELL, np.uint8)
            proofs = np.zeros(n * CELLS_PER_EXT_BLOB * 48, np.uint8)
            status = np.zeros(n, np.int32)
            self._check(self.lib.lb_kzg_compute_cells_and_proofs(self.engine.h, n, src.ctypes.data_as(u8), cells.ctypes.data_as(u8),
                                                                 proofs.ctypes.data_as(u8), status.ctypes.data_as(i32)), f"{what}Many")
            craw, praw = cells.tobytes(), proofs.tobytes()
            for b in range(n):
                if status[b] != 0:
                    res.append(KzgError(f"{what}: {self._N.error_name(int(status[b]))}"))
                    continue
                c0, p0 = b * CELLS_PER_EXT_BLOB * BYTES_PER_CELL, b * CELLS_PER_EXT_BLOB * 48
                res.append(([craw[c0 + BYTES_PER_CELL * i: c0 + BYTES_PER_CELL * (i + 1)] for i in range(CELLS_PER_EXT_BLOB)],
                            [praw[p0 + 48 * i: p0 + 48 * (i + 1)] for i in range(CELLS_PER_EXT_BLOB)]))
        return res

    def compute_cells_and_kzg_proofs(self, blob: bytes) -> Tuple[List[bytes], List[bytes]]:
        """c-kzg computeCellsAndKzgProofs: (the blob's 128 cells, their 128 proofs)"""
        res = self.compute_cells_and_kzg_proofs_many([blob])[0]
        if isinstance(res, KzgError):
            raise res
        return res

    def recover_cells_and_kzg_proofs_many(self, groups: Sequence[Tuple[Sequence[int], Sequence[bytes]]]) -> list:
        """recover_cells_and_kzg_proofs for many blobs (one group = one blob's cell indices and cells)
        in passes of up to 128 over the GPU (`lb_kzg_recover_cells_and_proofs`), whatever `field` is.
        One entry per blob: the pair (128 cells, 128 proofs), or the KzgError the single call would
        raise -- returned, not raised: BLST_BAD_SCALAR for a cell element >= r, and a failed check
        where more than 64 cells lie on no one polynomial of degree < 4096 (stricter than c-kzg).
        Malformed input raises ValueError before anything is sent: a wrong cell length, indices and
        cells of different lengths, fewer than 64 or more than 128 cells, an index outside 0 .. 127,
        indices that do not strictly ascend."""
        what = "recoverCellsAndKzgProofs"
        flat = []
        for g_idx, g_cells in groups:
            idx = [int(i) for i in g_idx]
            if len(idx) != len(g_cells):
                raise ValueError(f"{what}: {len(idx)} cell indices for {len(g_cells)} cells")
            if not CELLS_PER_EXT_BLOB // 2 <= len(idx) <= CELLS_PER_EXT_BLOB:
                raise ValueError(f"{what}: {len(idx)} cells, not {CELLS_PER_EXT_BLOB // 2} .. {CELLS_PER_EXT_BLOB}")
            if any(len(c) != BYTES_PER_CELL for c in g_cells):
                raise ValueError(f"{what}: {BYTES_PER_CELL}-byte cells")
            if any(not 0 <= i < CELLS_PER_EXT_BLOB for i in idx):
                raise ValueError(f"{what}: cell indices below {CELLS_PER_EXT_BLOB}")
            if any(a >= b for a, b in zip(idx, idx[1:])):
                raise ValueError(f"{what}: cell indices strictly ascending")
            flat.append((idx, [bytes(c) for c in g_cells]))
        u8, u32, i32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
        res: list = []
        for lo in range(0, len(flat), MAX_BLOBS_PER_CELLS_AND_PROOFS_CALL):
            part = flat[lo: lo + MAX_BLOBS_PER_CELLS_AND_PROOFS_CALL]
            n = len(part)
            off = np.cumsum([0] + [len(idx) for idx, _ in part]).astype(np.uint32)
            ci = np.asarray([i for idx, _ in part for i in idx], np.uint32)
            src = np.frombuffer(b"".join(c for _, g_cells in part for c in g_cells), np.uint8)
            cells = np.zeros(n * CELLS_PER_EXT_BLOB * BYTES_PER_CELL, np.uint8)
            proofs = np.zeros(n * CELLS_PER_EXT_BLOB * 48, np.uint8)
            status = np.zeros(n, np.int32)
            self._check(self.lib.lb_kzg_recover_cells_and_proofs(
                self.engine.h, n, off.ctypes.data_as(u32), ci.ctypes.data_as(u32), src.ctypes.data_as(u8), cells.ctypes.data_as(u8),
                proofs.ctypes.data_as(u8), status.ctypes.data_as(i32)), f"{what}Many")
            craw, praw = cells.tobytes(), proofs.tobytes()
            for b in range(n):
                if status[b] != 0:
                    res.append(KzgError(f"{what}: {self._N.error_name(int(status[b]))}"))
                    continue
                c0, p0 = b * CELLS_PER_EXT_BLOB * BYTES_PER_CELL, b * CELLS_PER_EXT_BLOB * 48
                res.append(([craw[c0 + BYTES_PER_CELL * i: c0 + BYTES_PER_CELL * (i + 1)] for i in range(CELLS_PER_EXT_BLOB)],
                            [praw[p0 + 48 * i: p0 + 48 * (i + 1)] for i in range(CELLS_PER_EXT_BLOB)]))
        return res

    def recover_cells_and_kzg_proofs(self, cell_indices: Sequence[int], cells: Sequence[bytes]) -> Tuple[List[bytes], List[bytes]]:
        """c-kzg recoverCellsAndKzgProofs: (all 128 cells, all 128 proofs) of the blob that any 64 .. 128
        of its cells, given with their strictly ascending indices, belong to"""
        res = self.recover_cells_and_kzg_proofs_many([(cell_indices, cells)])[0]
        if isinstance(res, KzgError):
            raise res
        return res

    def verify_cell_kzg_proof_batch_many(self, groups: Sequence[Tuple[Sequence[bytes], Sequence[int], Sequence[bytes], Sequence[bytes]]]) -> list:
        """verify_cell_kzg_proof_batch for many groups (one group = one call's commitments, cell
        indices, cells, proofs, one of each per cell) in one pass over the GPU
        (`lb_kzg_verify_cell_proof_batch`), whatever `field` is.  One entry per group: True, False, or
        the KzgError the single call would raise -- returned, not raised.  Malformed input (length
        mismatches, a wrong cell or point length, a cell index >= 128) raises before anything is sent."""
        what = "verifyCellKzgProofBatch"
        offsets, comms, idx, cells, proofs = [0], [], [], [], []
        for g_comms, g_idx, g_cells, g_proofs in groups:
            if not (len(g_comms) == len(g_idx) == len(g_cells) == len(g_proofs)):
                raise KzgError(f"{what}: commitments / cell indices / cells / proofs length mismatch")
            self._points48(what, g_comms, g_proofs)
            if any(len(c) != BYTES_PER_CELL for c in g_cells):
                raise KzgError(f"{what}: {BYTES_PER_CELL}-byte cells")
            if any(not 0 <= int(i) < CELLS_PER_EXT_BLOB for i in g_idx):
                raise KzgError(f"{what}: cell indices below {CELLS_PER_EXT_BLOB}")
            comms += [bytes(c) for c in g_comms]
            idx += [int(i) for i in g_idx]
            cells += [bytes(c) for c in g_cells]
            proofs += [bytes(p) for p in g_proofs]
            offsets.append(len(cells))
        n = len(offsets) - 1
        if n == 0:
            return []
        u8, u32, i32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
        cm = np.frombuffer(b"".join(comms) or b"\x00", np.uint8)
        ce = np.frombuffer(b"".join(cells) or b"\x00", np.uint8)
        pf = np.frombuffer(b"".join(proofs) or b"\x00", np.uint8)
        ci = np.asarray(idx or [0], np.uint32)
        off = np.asarray(offsets, np.uint32)
        ok = np.zeros(n, np.int32)
        self._check(self.lib.lb_kzg_verify_cell_proof_batch(
            self.engine.h, n, off.ctypes.data_as(u32), cm.ctypes.data_as(u8), ci.ctypes.data_as(u32), ce.ctypes.data_as(u8),
            pf.ctypes.data_as(u8), ok.ctypes.data_as(i32)), f"{what}Many")
        return [KzgError(f"{what}: {self._N.error_name(-int(v))}") if v < 0 else bool(v == 1) for v in ok]

    def verify_cell_kzg_proof_batch(self, commitments: Sequence[bytes], cell_indices: Sequence[int], cells: Sequence[bytes],
                                    proofs: Sequence[bytes]) -> bool:
        """c-kzg verifyCellKzgProofBatch: one group"""
        res = self.verify_cell_kzg_proof_batch_many([(commitments, cell_indices, cells, proofs)])[0]
        if isinstance(res, KzgError):
            raise res
        return res

    # the ckzg names kzg.ts binds
    computeCells = compute_cells
    computeCellsAndKzgProofs = compute_cells_and_kzg_proofs
    computeCellsAndKzgProofsMany = compute_cells_and_kzg_proofs_many
    recoverCellsAndKzgProofs = recover_cells_and_kzg_proofs
    recoverCellsAndKzgProofsMany = recover_cells_and_kzg_proofs_many
    verifyCellKzgProofBatch = verify_cell_kzg_proof_batch
    verifyCellKzgProofBatchMany = verify_cell_kzg_proof_batch_many
    computeBlobKzgProof = compute_blob_kzg_proof
    verifyBlobKzgProof = verify_blob_kzg_proof
    verifyBlobKzgProofBatch = verify_blob_kzg_proof_batch
    verifyBlobKzgProofBatchMany = verify_blob_kzg_proof_batch_many
    computeKzgProof = compute_kzg_proof_bytes
    verifyKzgProof = verify_kzg_proof_bytes
    verifyAggregateKzgProofBatch = verify_aggregate_kzg_proof_batch
    blobToKzgCommitment = blob_to_kzg_commitment
    computeAggregateKzgProof = compute_aggregate_kzg_proof
    verifyAggregateKzgProof = verify_aggregate_kzg_proof
    loadTrustedSetup = load_trusted_setup
