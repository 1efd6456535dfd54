"""No GPU: tests/tile_instances.py against the sources and against a restatement of the selection rules.

(a) every PRAM_NOTE_LAUNCH("family" in csrc/*.hip is a family of the table (and the other way round);
(b) every instantiation of the table has a case;
(c) the rules below — written from the dispatch code a second time, independently of the table — give every case the tag it
    claims.  They cross-check the table; on the GPU the tag the library reports is what counts (test_gpu_tile_instances.py)."""
import re
from pathlib import Path

import pytest

from tests import tile_instances as TI

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pram_amd" / "csrc"


def test_every_tagged_launch_site_is_in_the_table():
    found = set()
    calls = 0
    for src in sorted(CSRC.glob("*.hip")):
        text = src.read_text()
        calls += len(re.findall(r"\bPRAM_NOTE_LAUNCH\(", text))
        found |= set(re.findall(r'\bPRAM_NOTE_LAUNCH\("([^"]+)"', text))
    literal = sum(len(re.findall(r'\bPRAM_NOTE_LAUNCH\("', s.read_text())) for s in CSRC.glob("*.hip"))
    assert calls == literal, "a PRAM_NOTE_LAUNCH whose family is not a string literal hides from this test"
    assert found, "no tagged launch site found"
    assert found == set(TI.FAMILIES), found ^ set(TI.FAMILIES)
    # a launch by grid size without a record in front of it: every dispatch_tile lambda in the sources notes its launch
    for src in ("linear.hip", "conv.hip"):
        text = (CSRC / src).read_text()
        for m in re.finditer(r"dispatch_tile\(", text):
            body = text[m.end():m.end() + 700]
            body = body[:body.index("});") if "});" in body else len(body)]
            assert "PRAM_NOTE_LAUNCH" in body or "launch_linear_x3_t" in body, (src, body[:120])


def test_family_tags_are_well_formed():
    for fam, tags in TI.FAMILIES.items():
        base, _, variant = fam.partition("/")
        for tag in tags:
            assert re.fullmatch(re.escape(base) + r"<[a-z0-9,]+>", tag), tag
            assert not variant or tag.endswith("," + variant + ">"), (fam, tag)
    assert len(TI.all_tags()) == sum(len(t) for t in TI.FAMILIES.values()), "a tag listed under two families"


def test_every_instantiation_has_a_case():
    used = {c["tag"] for c in TI.CASES} | {c["tag_first"] for c in TI.CASES if "tag_first" in c}
    assert used <= TI.all_tags(), used - TI.all_tags()
    assert TI.all_tags() <= used, sorted(TI.all_tags() - used)
    for c in TI.CASES:
        assert c["bar"] in TI.BARS, c
    ids = [TI.case_id(c) for c in TI.CASES]
    assert len(set(ids)) == len(ids)


def test_bars_quote_existing_assertions():
    """every bar is the number on the quoted line of the existing test"""
    for name, (value, where) in TI.BARS.items():
        path, line = where.rsplit(":", 1)
        text = (ROOT / path).read_text().splitlines()[int(line) - 1]
        assert "assert" in text, (name, where, text)
        numbers = {float(x) for x in re.findall(r"\d+(?:\.\d+)?e-\d+", text)} | {2.0 ** -int(x) for x in re.findall(r"2\.0 \*\* -(\d+)", text)}
        assert value in numbers, (name, value, where, text)


def test_epilogues_cover_every_x3_linear_instantiation():
    for tag in list(TI.FAMILIES["linear_x3"]) + list(TI.FAMILIES["linear_x3w"]):
        have = {c["epi"] for c in TI.CASES if c["entry"] == "linear" and c["tag"] == tag}
        assert set(TI.EPILOGUES) <= have, (tag, have)
    for entry, fams in (("linear_planes", ("linear_x3p", "linear_x3w/planes")), ("linear_qkv_planes", ("linear_x3", "linear_x3w")),
                        ("mlp_tail", ("linear_x3/lngelu", "linear_x3w/lngelu"))):
        want = {t for f in fams for t in TI.FAMILIES[f]}
        if entry == "linear_qkv_planes":
            want -= {"linear_x3<1,1>", "linear_x3<2,1>"}      # n >= 128: a q column block and a value head
        have = {c["tag"] for c in TI.CASES if c["entry"] == entry}
        assert want <= have, (entry, want - have)
    firsts = {c["tag_first"] for c in TI.CASES if c["entry"] == "mlp_tail"}
    assert {"linear_x3<2,1>", "linear_x3<2,2>", "linear_x3w<2,2,4>", "linear_x3w<4,2,4>"} <= firsts
    for c in TI.CASES:
        if c["entry"] == "conv":
            twin = dict(c, form="full" if c["form"] == "plain" else "plain")
            assert twin in TI.CASES, c


# ------------------------------------------------------------------------------------------------ (c) the rules, restated
def cdiv(a, b):
    return -(-a // b)


def choose_tile(m, n):
    wn = 1 if n <= 64 else 2
    blocks = cdiv(m, (4 // wn) * 64) * cdiv(n, wn * 64)
    return (2 if blocks >= 512 else 1), wn


def wide_tile(m, n, k, batch=1):
    """(MI, WM, WN) of the wide split-fp16 tile, or None: the choose_tile ladder"""
    if n < 256 or k % 32:
        return None
    big, small = cdiv(m, 256) * cdiv(n, 256) * batch, cdiv(m, 128) * cdiv(n, 256) * batch
    if small < 192:
        return None
    return (4, 2, 4) if big >= 224 and 100 * cdiv(big, 256) <= 55 * cdiv(small, 256) else (2, 2, 4)


def split_linear(m, n, k, planes, batch=1, variant=""):
    v = "," + variant if variant else ""
    w = wide_tile(m, n, k, batch)
    if w:
        return "linear_x3w<%d,%d,%d%s>" % (*w, ",planes" if planes else v)
    mi, wn = choose_tile(m, n)
    return ("linear_x3p<%d,%d>" % (mi, wn)) if planes else ("linear_x3<%d,%d%s>" % (mi, wn, v))


def f32_linear(rows, n):
    mi, wn = choose_tile(rows, n)
    return "linear_f32<%d,%d,%d>" % (mi, wn, 16 if mi == 2 else 32)


def predict_linear(c):
    m, n, k = c["m"], c["n"], c["k"]
    if c["epi"] == "lens":
        m = cdiv(m, 1024) * 1024      # as the runner pads: whole sequences
    if c["prec"] == "x3":
        assert k % 32 == 0
        return split_linear(m, n, k, False)
    if c["prec"] == "f16":
        assert k % 64 == 0
        mi, wn = choose_tile(m, n)
        return "linear_f16<%d,%d>" % (1 if wn == 1 else mi, wn)
    return f32_linear(m, n)


def predict_conv(c):
    b, h, w = c["bhw"]
    ks, st, cin, cout = c["ks"], c["stride"], c["cin"], c["cout"]
    ho, wo = (h + 2 * (ks // 2) - ks) // st + 1, (w + 2 * (ks // 2) - ks) // st + 1
    m = b * ho * wo
    mi, wn = choose_tile(m, cout)
    if c["prec"] == "x3" and cin % 32 == 0:
        if ks == 3 and st == 1 and (cout >= 256 or cout == 128):
            if b * cdiv(wo, 32) * cdiv(ho, 8) * cdiv(cout, 128 if cout <= 128 else 256) >= 224:
                return "conv_x3h<%d>" % (2 if cout <= 128 else 4)
        if cout >= 256 and cdiv(m, 256) * cdiv(cout, 256) >= 224:
            return "conv_x3w<4,2,4>"
        return "conv_x3<%d,%d>" % (mi, wn)
    if c["prec"] == "f16" and cin % 64 == 0:
        return "conv_f16<%d,%d>" % (mi, wn)
    if cin == 4:
        return "conv_f32_cin4<2,%d,16>" % wn
    return "conv_f32<%d,%d,%d>" % (mi, wn, 16 if wn == 1 else 32)


def predict_attention(c, heads=4):
    b, m, n = c["batch"], c["m"], c["n"]
    units256 = b * heads * cdiv(m, 256)
    if c["entry"] == "attention_h16t":
        return "attention_h16t<%d>" % (8 if units256 >= 256 else 4)
    if n < 1024:
        return "attention_x3_pipe<ps,mode0," + ("w8,phases>" if units256 >= 256 else "w4,interleaved>")
    ps = "ps" if c.get("p_split", 1) else "p1"
    chunk = c.get("chunk", 4096)
    nchunks = cdiv(n, chunk)
    if nchunks < 2:
        return "attention_x3_pipe<%s,mode0," % ps + ("w8,phases>" if units256 >= 256 else "w4,interleaved>")
    units = b * heads * cdiv(m, 128)
    groups = 1
    if c.get("split", True):
        g = c.get("target", 256) // units
        groups = 1 if g < 2 else min(g, nchunks)
    if groups < 2:
        phases = units >= 512 and cdiv(n, 64) >= 32
        return "attention_x3_pipe<%s,mode1,w4,%s>" % (ps, "phases" if phases else "interleaved")
    group_tiles = cdiv(nchunks, groups) * (chunk // 64)
    nsplit = cdiv(nchunks * (chunk // 64), group_tiles)
    phases = units * nsplit >= 512 and group_tiles >= 32
    return "attention_x3_pipe<%s,mode2,w4,%s>" % (ps, "phases" if phases else "interleaved")


def predict(c):
    e = c["entry"]
    if e == "linear":
        return predict_linear(c)
    if e == "linear_planes":
        return split_linear(c["m"], c["n"], c["k"], True)
    if e == "linear_qkv_planes":
        return split_linear(c["m"], c["n"], c["k"], False)
    if e == "mlp_tail":
        return split_linear(c["m"], c["n"], c["hid"], False, variant="lngelu")
    if e == "bgemm_nt":
        return f32_linear(c["m"] * c["batch"], c["n"])
    if e == "bgemm_nt_planes":
        return split_linear(c["m"], c["n"], c["k"], True, batch=c["batch"])
    if e == "conv":
        return predict_conv(c)
    return predict_attention(c)


@pytest.mark.parametrize("case", TI.CASES, ids=TI.case_id)
def test_rules_predict_the_tag_of_every_case(case):
    assert predict(case) == case["tag"]
    if case["entry"] == "mlp_tail":
        assert split_linear(case["m"], case["hid"], case["k"], False) == case["tag_first"]


def test_threshold_shapes_sit_on_the_threshold():
    """the smallest shapes: one row fewer than the rule asks for lands on the smaller instantiation"""
    assert choose_tile(130817, 64) == (2, 1) and choose_tile(130816, 64) == (1, 1)
    assert choose_tile(32641, 136) == (2, 2) and choose_tile(32640, 136) == (1, 2)
    assert choose_tile(65409, 128) == (2, 2) and choose_tile(65408, 128) == (1, 2)
    assert wide_tile(24449, 256, 64) == (2, 2, 4) and wide_tile(24448, 256, 64) is None
    assert wide_tile(57089, 256, 64) == (4, 2, 4) and wide_tile(57088, 256, 64) == (2, 2, 4)
    assert wide_tile(28417, 264, 64) == (4, 2, 4) and wide_tile(28416, 264, 64) == (2, 2, 4)
    assert wide_tile(100, 256, 64, 192) == (2, 2, 4) and wide_tile(100, 256, 64, 191) is None
    assert wide_tile(130, 256, 64, 224) == (4, 2, 4) and wide_tile(130, 256, 64, 223) == (2, 2, 4)
