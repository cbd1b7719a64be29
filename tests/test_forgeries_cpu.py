"""tests/golden/forgeries.json against the pure-Python oracle: the forged groups are real attacks on
an unblinded batch check (each set alone is invalid and in G2; the group passes with equal scalars,
the triple with an affine sequence too; unrelated scalars reject it), and the negated pair is valid
under any scalars.  Also oracle_partial(), the batch's Fp12 product before the final exponentiation
as the oracle computes it from blinding words, which tests/test_forgeries_gpu.py compares the
device's partials with."""
import collections
import functools

import pytest

from conftest import load_json
from oracle import bls_oracle as o

Set = collections.namedtuple("Set", "pubkeys signing_root signature")  # the fields of engine.SetInput

FORGED = {"pair_same_root": [3, 5], "triple_same_root": [3, 5, 11], "pair_aggregate": [3, 5],
          "pair_sibling_roots": [3, 5]}


def group(name):
    """the named group of the fixture as Sets of bytes"""
    return [Set([bytes.fromhex(p) for p in s["pubkeys"]], bytes.fromhex(s["signing_root"]), bytes.fromhex(s["signature"]))
            for s in load_json("forgeries.json")["groups"][name]]


_hash_to_g2 = o.hash_to_g2


# shared oracle values, each computed once per process: H(m) per root, decoded keys and signatures
@functools.lru_cache(maxsize=None)
def hashed(m):
    return _hash_to_g2(m, o.DST_POP)


@functools.lru_cache(maxsize=None)
def _decoded(pubkeys, signature):
    pk = None
    for k in pubkeys:
        pk = o.g1_add(pk, o.g1_deserialize(k))
    return pk, o.signature_from_bytes(signature, True)  # raises unless the signature is in G2


def decoded(s):
    """(aggregate pubkey, signature) as affine points"""
    return _decoded(tuple(bytes(k) for k in s.pubkeys), bytes(s.signature))


def oracle_partial(sets, words, plain=False):
    """prod ML(r_i PK_i, H(m_i)) * ML(-G1, sum r_i sig_i) with r_i = blinding_scalar(word_i), the value
    whose final exponentiation decides the batch (plain: r_i = word_i, the 64-bit integer itself)"""
    f, ssum = o.F12_ONE, None
    for s, w in zip(sets, words):
        r = int(w) if plain else o.blinding_scalar(int(w))
        pk, sig = decoded(s)
        ssum = o.g2_add(ssum, o.g2_mul(sig, r))
        f = o.f12_mul(f, o.miller_loop(o.g1_mul(pk, r), hashed(bytes(s.signing_root))))
    return o.f12_mul(f, o.miller_loop(o.g1_neg(o.G1), ssum))


@pytest.fixture(scope="module", autouse=True)
def shared_hashes():
    """verify_multiple_signatures and core_verify hash every message anew: serve them from the cache"""
    mp = pytest.MonkeyPatch()
    mp.setattr(o, "hash_to_g2", lambda m, dst=o.DST_POP: hashed(m) if dst == o.DST_POP else _hash_to_g2(m, dst))
    yield
    mp.undo()


def triples(sets):
    return [(decoded(s)[0], s.signing_root, decoded(s)[1]) for s in sets]


@pytest.mark.parametrize("name", sorted(FORGED))
def test_forged_group_cancels_only_unblinded(name):
    sets = group(name)
    t = triples(sets)
    for pk, m, sig in t:
        assert o.g2_in_subgroup(sig)
        assert not o.core_verify(pk, m, sig)
    assert o.verify_multiple_signatures(t, scalars=[1] * len(t))
    if len(t) == 3:
        assert o.verify_multiple_signatures(t, scalars=[1, 2, 3])
    assert not o.verify_multiple_signatures(t, scalars=FORGED[name])


def test_negated_valid_pair_is_valid_under_any_scalars():
    t = triples(group("negated_valid_pair"))
    assert t[1][0] == o.g1_neg(t[0][0]) and t[1][1] == t[0][1] and t[1][2] == o.g2_neg(t[0][2])
    for pk, m, sig in t:
        assert o.core_verify(pk, m, sig)
    assert o.verify_multiple_signatures(t, scalars=[7, 7])
    assert o.verify_multiple_signatures(t, scalars=[3, 5])


def test_edge_words_sets_six_valid_one_wrong_message():
    sets = group("edge_words")
    assert len({s.signing_root for s in sets}) == 7
    assert [o.core_verify(pk, m, sig) for pk, m, sig in triples(sets)] == [True] * 6 + [False]


def test_oracle_partial_decides_as_verify_multiple_signatures():
    """FE(oracle_partial) is one exactly when the oracle's batch check with r = blinding_scalar(word) passes"""
    sets = group("pair_same_root")
    assert o.final_exponentiation(oracle_partial(sets, [1, 1])) == o.F12_ONE
    words = [0x0000000500000003, 0xFFFFFFFF00000001]
    assert o.final_exponentiation(oracle_partial(sets, words)) != o.F12_ONE
    assert not o.verify_multiple_signatures(triples(sets), scalars=[o.blinding_scalar(w) for w in words])
