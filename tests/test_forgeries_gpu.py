"""Soundness of the blinding on the device: forged sets whose errors cancel under an unblinded (or
affinely weighted) sum, planted inside one batch at the places where each step of the verifier and
of the invalid-set search sums sets, and edge blinding words against the oracle, form by form.

tests/golden/forgeries.json (tests/golden/make_forgeries.py; checked on the CPU by
tests/test_forgeries_cpu.py) and tests/golden/cancel_pair.json hold signatures sk H(m) + k D whose
offsets sum to zero inside a group.  Every other invalid set this suite plants is an honest error (a
signature over another message), which any linear combination exposes: a step that dropped the
blinding words, used one word per root, or weighted sets only by the search's c + 1 would still
reject those.  It accepts these.  Expected values come from the fixture and the oracle alone; the
byte-identity of the partials across forms stands beside the oracle equality, not in its place."""
import hashlib
import re

import numpy as np
import pytest

import test_forgeries_cpu as FC
from conftest import load_json
from lodestar_amd.engine import PackedJobs, SetInput, pack_jobs

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
BIG = str(1 << 31)


def interop_sk(i):
    d = hashlib.sha256(i.to_bytes(32, "little")).digest()
    return int.from_bytes(d, "little") % R


def fresh_root(i):
    return hashlib.sha256(b"forgery-filler-root-%d" % i).digest()


def fixture(name):
    return [SetInput(*s) for s in FC.group(name)]


def cancel_pair():
    return [SetInput([bytes.fromhex(s["pubkey"])], bytes.fromhex(s["signing_root"]), bytes.fromhex(s["signature"]))
            for s in load_json("cancel_pair.json")["sets"]]


def fillers(engine, roots, agg_k=1):
    """one valid set per entry of `roots`, signed on the GPU under interop keys 24.. (the fixture's are 3..23)"""
    pool = [interop_sk(24 + i) for i in range(40)]
    _, pk96 = engine.sk_to_pk(pool)
    idx = [[(7 * i + 3 * j) % 40 for j in range(agg_k)] for i in range(len(roots))]
    sks = [sum(pool[j] for j in row) % R for row in idx]
    sigs = engine.sign(sks, np.frombuffer(b"".join(roots), np.uint8).reshape(-1, 32))
    return [SetInput([pk96[j].tobytes() for j in row], m, sigs[i].tobytes()) for i, (row, m) in enumerate(zip(idx, roots))]


def planted(engine, roots, forged, agg_k=1):
    """single-set jobs over `roots` in input order; forged: {position: set} replaces the filler there"""
    sets = fillers(engine, roots, agg_k)
    for p, s in forged.items():
        assert s.signing_root == roots[p]
        sets[p] = s
    return [[s] for s in sets]


class Shape:
    def __init__(self, jobs, bad_jobs, bad_sets=None):
        self.packed = pack_jobs(jobs)
        self.expected = [0 if j in bad_jobs else 1 for j in range(len(jobs))]
        self.bad_sets = sorted(bad_jobs if bad_sets is None else bad_sets)
        seen = {}
        self.roots = np.array([seen.setdefault(s.signing_root, len(seen)) for j in jobs for s in j], dtype=np.uint32)
        n = self.packed.n_sets
        # pinned words: pairwise distinct, odd, over the whole 64-bit range (top bit of hi included)
        self.words = np.random.default_rng(0xF0 + n).integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        assert len(set(self.words.tolist())) == n


_SHAPES = {}


def shapes(engine):
    """The batches, made once per module.  The fillers are signed through the session `engine` fixture
    and the packed batches are reused on every engine below: the knobs change how an engine verifies,
    not what sign returns."""
    if _SHAPES:
        return _SHAPES
    pair, triple, agg, sib, cp = (fixture("pair_same_root"), fixture("triple_same_root"), fixture("pair_aggregate"),
                                  fixture("pair_sibling_roots"), cancel_pair())
    (valid,) = fillers(engine, [fresh_root(0)])
    # A: the root check (2 sets, 2 roots)
    _SHAPES["A"] = Shape([[cp[0]], [cp[1]]], {0, 1})
    # B: the per-root sum (2 sets, 1 root); the job's own verdict (one 2-set job beside a valid job)
    _SHAPES["B"] = Shape([[pair[0]], [pair[1]]], {0, 1})
    _SHAPES["B_job"] = Shape([pair, [valid]], {0}, bad_sets={0, 1})
    # C: the per-root sum and a c + 1 weighted test over the root's three single-set parts
    _SHAPES["C"] = Shape([[triple[0]], [triple[1]], [triple[2]], [valid]], {0, 1, 2})
    # D: a root of 130 members (input positions 0..129, members keep input order): a weighted test over
    # 130 single-set parts, then direct checks of parts of 3 sets; the triple fills part 7
    big = triple[0].signing_root
    roots = [big] * 130 + [fresh_root(1)] * 2 + [fresh_root(2)] * 2
    _SHAPES["D"] = Shape(planted(engine, roots, {21: triple[0], 22: triple[1], 23: triple[2]}), {21, 22, 23})
    # E: a root of 1100 members (> LB_WT_MAX = 1024): weighted parts of two sets; the pair fills part 200
    roots = [pair[0].signing_root] * 1100 + [fresh_root(3)] * 3
    _SHAPES["E"] = Shape(planted(engine, roots, {400: pair[0], 401: pair[1]}), {400, 401})
    # F: 130 single-member roots; in input order (LB_ROOT_SHUFFLE=0) the root numbers are the positions,
    # so each pair sits inside one 64-root subtree: roots 10, 11 and roots 82, 83
    roots = [fresh_root(10 + i) for i in range(130)]
    for p, s in ((10, cp[0]), (11, cp[1]), (82, sib[0]), (83, sib[1])):
        roots[p] = s.signing_root
    _SHAPES["F"] = Shape(planted(engine, roots, {10: cp[0], 11: cp[1], 82: sib[0], 83: sib[1]}), {10, 11, 82, 83})
    # G: the aggregate-key path: the pair over two keys each among 20 valid two-key sets, 10 on its root
    roots = [agg[0].signing_root] * 12 + [fresh_root(200 + i // 2) for i in range(10)]
    _SHAPES["G"] = Shape(planted(engine, roots, {4: agg[0], 9: agg[1]}, agg_k=2), {4, 9})
    return _SHAPES


def indexed(e, packed):
    """the same batch with its keys registered in the engine's resident table, as table indices"""
    keys = np.ascontiguousarray(packed.pubkeys).reshape(-1, 96)
    uniq, inverse = np.unique(keys, axis=0, return_inverse=True)
    first, st = e.pubkey_table_append(np.ascontiguousarray(uniq))
    assert not any(st)
    return PackedJobs(job_off=packed.job_off, pk_off=packed.pk_off, pubkeys=None, msgs=packed.msgs, sigs=packed.sigs,
                      sig_sizes=packed.sig_sizes, pk_indices=(first + inverse.reshape(-1)).astype(np.uint32))


def check_shape(e, name, sh, by_index=False):
    """exactly the forged jobs are rejected under the engine's own words and under pinned distinct ones;
    A-C: with every word 1 the batch is accepted at the root check (the oracle's answer: the control)"""
    b = e.upload(indexed(e, sh.packed) if by_index else sh.packed)
    try:
        assert b.verify().tolist() == sh.expected, (name, "engine words")
        assert b.verify(scalars=sh.words).tolist() == sh.expected, (name, "pinned words")
        if name in ("A", "B", "B_job", "C"):
            e.set_profiling(True)
            try:
                ones = b.verify(scalars=np.ones(b.n_sets, dtype=np.uint64)).tolist()
                prof = e.last_profile()
            finally:
                e.set_profiling(False)
            assert ones == [1] * b.n_jobs, (name, "every word 1")
            assert prof["search_msm"] == 0.0, name
        if name == "D":
            _, st = b.partial()
            assert st.tolist() == [1] * b.n_jobs
            assert b.search_after_partial(fallback=False).tolist() == sh.expected, (name, "after partial")
    finally:
        b.free()


KNOBS = [
    {"LB_ALONE": "1"},
    {"LB_ALONE": "0"},
    {"LB_SMSM_FORM": "lane"},
    {"LB_SEARCH_SMALL_MAX": "0"},                                                       # bucket MSM rounds
    {"LB_SEARCH_SMALL_MAX": "0", "LB_SEARCH_BLOCKS": "0"},                              # per-root sums
    {"LB_SEARCH_SMALL_MAX": "0", "LB_SEARCH_BLOCKS": "0", "LB_SEARCH_ROOTSUM": "0"},
    {"LB_SEARCH_MERGE": "0"},
    {"LB_SEARCH_CHUNK": "1"},
    # one-lane and MSM root forms
    {"LB_SUBGROUP_G8_MAX": "0", "LB_SMALL_S_MAX": "0", "LB_MILLER_WAVE_MAX": "0", "LB_HASH_G8_MAX": "0"},
]


def knob_id(k):
    return "+".join("%s=%s" % kv for kv in k.items())


@pytest.mark.parametrize("knobs", KNOBS, ids=knob_id)
def test_forgeries_rejected_in_every_search_form(engine, monkeypatch, knobs):
    """Shapes A-G through one engine per knob set (an engine reads the knobs when it is created)."""
    from lodestar_amd.engine import Engine
    S = shapes(engine)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    with Engine(0) as e:
        for name, sh in S.items():
            check_shape(e, name, sh)


def test_forgeries_rejected_with_comb_blinded_keys(engine, monkeypatch):
    """Shapes C and D uploaded as table indices under load (LB_ALONE=0) with the fixed-base comb on, so
    k_pk_blind_comb computes r PK of the forged single-key sets."""
    from lodestar_amd.engine import Engine
    S = shapes(engine)
    monkeypatch.setenv("LB_ALONE", "0")
    monkeypatch.setenv("LB_PK_COMB", "1")
    with Engine(0) as e:
        for name in ("C", "D"):
            check_shape(e, name, S[name], by_index=True)
        assert e.pubkey_comb_sets() > 0


@pytest.mark.parametrize("alone", ["0", "1"])
def test_forged_parts_exist_as_the_plan_model_says(engine, monkeypatch, capfd, alone):
    """With the roots in input order (LB_ROOT_SHUFFLE=0) the CPU model of the search (tests/test_search_plan_cpu.py),
    given the forged positions as failing sets, predicts the rounds of D, E and F, and the device's trace
    equals them: so the parts meant to hold a whole cancelling group were checked.  D: 3 root checks; 44
    direct checks of parts of 3 sets (part 7 is the triple); 3 single sets.  E: the weighted test over 550
    parts of two sets names part 200 (the pair), whose own test matches nothing; 2 single sets.  F: 3
    subtree checks, two of them over a whole pair; then the 128 roots of the two failing subtrees."""
    import test_search_plan_cpu as SP
    from lodestar_amd.engine import Engine
    S = shapes(engine)
    monkeypatch.setenv("LB_ROOT_SHUFFLE", "0")
    monkeypatch.setenv("LB_SEARCH_TRACE", "1")
    monkeypatch.setenv("LB_ALONE", alone)
    lib = SP.load()
    with Engine(0) as e:
        for name, checks in (("D", [3, 44, 3]), ("E", [2, 0, 2]), ("F", [3, 128])):
            sh = S[name]
            found, model, _ = SP.run(lib, sh.roots, sh.bad_sets, flags=SP.SPEC if alone == "1" else 0)
            assert sorted(found) == sh.bad_sets
            assert [row[2] for row in model] == checks, (name, model)
            capfd.readouterr()
            assert e.verify_jobs_packed(sh.packed) == sh.expected, name
            err = capfd.readouterr().err
            got = [[int(v) for v in m.groups()] for m in re.finditer(
                r"\[lb search\] round (\d+): (\d+) failing nodes, (\d+) direct checks, (\d+) weighted tests", err)]
            assert got == [row[:4] for row in model], (name, got, model)
            assert name != "D" or got[-1][0] >= 2   # at least two search rounds ran


# ---------------------------------------------------------------- edge words against the oracle
EDGE_WORDS = [0x0000000000000001,
              0x00000000FFFFFFFF,   # hi = 0
              0xFFFFFFFF00000000,   # lo = 0: r = hi * lambda
              0xFFFFFFFFFFFFFFFF,   # every 8-bit window digit 255, the top comb digit
              0x8000000080000000,   # only the top bit of each half
              0x0000000100000000,   # r = lambda
              0x0001000000000100]   # zero bottom window
PAIR_WORD = 0xDEADBEEF12345677      # on both sets of the negated pair: the root's sum r PK is infinity

FORMS = {
    "alone": {"LB_ALONE": "1"},                                                    # row forms
    "load": {"LB_ALONE": "0"},
    "lane": dict(LB_ALONE="0", LB_MILLER_WAVE_MAX="0", LB_HASH_G8_MAX="0", LB_SUBGROUP_G8_MAX="0", LB_SMALL_S_MAX="0",
                 LB_SMALL_S_G8_MAX="0", LB_SEARCH_SMALL_MAX="0"),                  # one-lane forms, bucket MSM for S
    "many": dict(LB_ALONE="0", LB_MILLER_WAVE_MAX=BIG, LB_HASH_G8_MAX=BIG, LB_SUBGROUP_G8_MAX=BIG, LB_SMALL_S_MAX=BIG,
                 LB_SMALL_S_G8_MAX=BIG, LB_SEARCH_SMALL_MAX=BIG),                  # many-lane forms
    "lane_msm_lone": dict(LB_ALONE="0", LB_MSM_G8="0", LB_MILLER_WAVE_MAX="0", LB_HASH_G8_MAX="0", LB_SUBGROUP_G8_MAX="0",
                          LB_SMALL_S_MAX="0", LB_SMALL_S_G8_MAX="0", LB_SEARCH_SMALL_MAX="0"),
    "comb": {"LB_ALONE": "0", "LB_PK_COMB": "1"},                                  # the indexed upload
}


def edge_sets():
    """the seven sets of edge_words (six valid, the last signed over another root), then the negated pair"""
    return fixture("edge_words") + fixture("negated_valid_pair")


def edge_words(k):
    """the edge words turned by k places over the first seven sets (k = 0: as listed), the pair's shared word"""
    return np.array(EDGE_WORDS[-k:] + EDGE_WORDS[:-k] + [PAIR_WORD] * 2 if k else EDGE_WORDS + [PAIR_WORD] * 2,
                    dtype=np.uint64)


def fe_of(raw):
    """the final exponentiation of a 576-byte partial, as the oracle's Fp12 value"""
    vals = [int.from_bytes(raw[48 * k:48 * (k + 1)], "big") for k in range(12)]
    f = tuple(tuple((vals[6 * a + 2 * c], vals[6 * a + 2 * c + 1]) for c in range(3)) for a in range(2))
    return FC.o.final_exponentiation(f)


_ORACLE = {}


def edge_oracle(key):
    """Each once per module (seconds of Python).  base / plain: FE of the oracle's partial over all nine sets
    with the words as listed, read as r = lo + hi * lambda and as plain integers.  turned: for the words
    turned by k = 0..6 places; a valid set's factor ML(r PK, H(m)) ML(-G1, r sig) is one after the final
    exponentiation whatever r is (k = 0 is checked against base, over all nine), so that value is the
    oracle's partial of the wrong-message set alone under the word it then carries."""
    if key not in _ORACLE:
        o, sets = FC.o, edge_sets()
        if key == "turned":
            _ORACLE[key] = [o.final_exponentiation(FC.oracle_partial(sets[6:7], edge_words(k)[6:7])) for k in range(7)]
            assert _ORACLE[key][0] == edge_oracle("base")
        else:
            _ORACLE[key] = o.final_exponentiation(FC.oracle_partial(sets, edge_words(0), plain=key == "plain"))
    return _ORACLE[key]


_EDGE_RUNS = {}


def edge_run(form):
    """(codes of verify under the listed words, statuses of partial, the partials under the words turned by
    0..6 places) of the nine-set batch on an engine created with the form's knobs; once per form"""
    if form not in _EDGE_RUNS:
        from lodestar_amd.engine import Engine
        packed = pack_jobs([[s] for s in edge_sets()])
        with pytest.MonkeyPatch.context() as mp:
            for k, v in FORMS[form].items():
                mp.setenv(k, v)
            with Engine(0) as e:
                b = e.upload(indexed(e, packed) if form == "comb" else packed)
                try:
                    codes = b.verify(scalars=edge_words(0)).tolist()
                    raws, sts = zip(*[b.partial(edge_words(k)) for k in range(7)])
                finally:
                    b.free()
                assert form != "comb" or e.pubkey_comb_sets() > 0
        _EDGE_RUNS[form] = (codes, [st.tolist() for st in sts], list(raws))
    return _EDGE_RUNS[form]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_edge_words_partial_matches_oracle(form):
    """Nine sets, one per job: six valid sets and one wrong-message set under the edge words, and a valid
    pair (PK, m, sig), (-PK, m, -sig) under one shared word, whose root sum r PK - r PK is the point at
    infinity (k_gsum_final's gp_inf by cancellation).  FE(partial) equals FE of the oracle's product with
    r = blinding_scalar(word), is not one, differs from the oracle's with the words as plain integers, and
    verify rejects exactly the wrong-message job."""
    codes, sts, raws = edge_run(form)
    assert sts == [[1] * 9] * 7
    got = fe_of(raws[0])
    assert got == edge_oracle("base")
    assert got != FC.o.F12_ONE
    assert got != edge_oracle("plain")
    assert codes == [1] * 6 + [0] + [1, 1]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_edge_words_each_on_the_wrong_message_set(form):
    """After the final exponentiation only the wrong-message set's r is left in the value above (the valid
    sets' r must merely be the same on the key and on the signature side).  So the words take turns: each
    edge word once on the wrong-message set, each partial against the oracle."""
    want = edge_oracle("turned")
    raws = edge_run(form)[2]
    for k in range(1, 7):
        assert fe_of(raws[k]) == want[k], (form, "word %#018x on the wrong-message set" % int(edge_words(k)[6]))


def test_edge_words_partials_byte_identical_across_forms():
    """the forms-agree comparison on a failing batch and on words with the top bit set"""
    runs = {form: edge_run(form)[2] for form in sorted(FORMS)}
    first = runs["alone"]
    for form, raws in runs.items():
        assert raws == first, (form, [k for k in range(7) if raws[k] != first[k]])
