"""The library's environment switches, no GPU needed: one table (csrc/tdx_ordered.hip) behind tdx_switch_count / _name /
_default / _value, one parser, every switch read per call, Python asking the library instead of parsing on its own, and the
documents and sources agreeing with the table.  Nothing is launched."""

import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "generative-turbulence_amd" / "csrc"

# Every value INTEGRATION.md section 5 documents (and the defaults), per switch: each must come back as it was set.  A switch
# added to the library fails test_documented_values_come_back until it has a row here.
DOCUMENTED = {
    "TDX_ATTN_BOUND": (0, 1),
    "TDX_ATTN_BWD_TW": (11, 12, 21, 22),
    "TDX_ATTN_IMPL": (0, 1),
    "TDX_ATTN_STREAMK": (0, 1),
    "TDX_CONV1_IMPL": (0, 1),
    "TDX_CONV3_PERM": (0, 1),
    "TDX_CONV3_RING": (0, 1, 2),
    "TDX_CONV3_SMALL": (0, 1),
    "TDX_CONV3_SMALL_ROWS": (0, 1, 6000, 30000),
    "TDX_CONV3_THIN": (0, 1, 2),
    "TDX_CONVG_MFMA": (0, 1),
    "TDX_DETERMINISTIC": (0, 1),
    "TDX_PERSISTENT_CUS": (8, 64, 192, 224, 256),
    "TDX_RING_LOADERS": (0, 1),
    "TDX_RING_MIN_ITEMS": (0, 1, 768, 100000),
    "TDX_RING_RAGGED": (0, 1),
    "TDX_RING_Z4": (0, 1, 2),
    "TDX_SHELL_DETERMINISTIC": (0, 1),
    "TDX_SKIP_DGRAD_FUSE": (0, 1),
    "TDX_SMALL_ZPAD": (0, 1),
    "TDX_WGRAD_RING": (0, 1, 2),
    "TDX_WGRAD_SMALL": (0, 1),
    "TDX_WGRAD_SMALL_ROWS": (0, 1, 8000, 30000),
    "TDX_WGRAD_SPLIT_RING": (0, 1),
}
WORDS = {"TDX_CONV1_IMPL": "direct", "TDX_ATTN_IMPL": "vector"}


@pytest.fixture
def L(monkeypatch):
    """turbdiff_amd._lib with every library switch cleared (the suite also runs with TDX_DETERMINISTIC=1 exported)."""
    from turbdiff_amd import _lib

    for name in _lib.switch_names():
        monkeypatch.delenv(name, raising=False)
    return _lib


def test_table_sanity(L):
    names = L.switch_names()
    assert len(names) == len(set(names)) == L.load().tdx_switch_count() >= 24
    assert all(re.fullmatch(r"TDX_[A-Z0-9_]+", n) for n in names)
    for n in names:
        assert L.switch(n) == L.switch_default(n), n  # cleared: the default
    # every default is among the row's accepted values (the library also asserts it over the whole table at compile time)
    assert set(names) == set(DOCUMENTED)
    for n in names:
        assert L.switch_default(n) in DOCUMENTED[n], n
    lib = L.load()
    for i in (-1, len(names)):
        assert lib.tdx_switch_name(i) is None and lib.tdx_switch_default(i) == 0 and lib.tdx_switch_value(i) == 0


def test_documented_values_come_back(L, monkeypatch):
    assert set(L.switch_names()) == set(DOCUMENTED), "a library switch without a row in DOCUMENTED (or the reverse)"
    for n, values in DOCUMENTED.items():
        for v in values:
            monkeypatch.setenv(n, str(v))
            assert L.switch(n) == v, (n, v)
        monkeypatch.delenv(n)
        assert L.switch(n) == L.switch_default(n), n


def test_one_parser(L, monkeypatch):
    for n in L.switch_names():
        d = L.switch_default(n)
        other = next(v for v in DOCUMENTED[n] if v != d)
        # not a whole decimal integer (nor the row's word): as if unset, whatever the string begins with
        for s in ("", "off", "x", f"{other}x", f"{other} ", f"{other}.0", "0x1", "direct-ish", "vectors"):
            monkeypatch.setenv(n, s)
            assert L.switch(n) == d, (n, s)
        if n == "TDX_PERSISTENT_CUS":
            continue
        for s in ("-1", "2147483648", "99999999999999999999"):  # out of every row's range
            monkeypatch.setenv(n, s)
            assert L.switch(n) == d, (n, s)
    for s, want in (("300", 256), ("4", 8), ("100", 96), ("-5", 8), ("224", 224), ("231", 224), ("", 256), ("many", 256)):
        monkeypatch.setenv("TDX_PERSISTENT_CUS", s)  # the one row that clamps; used rounded down to a multiple of 8
        assert L.switch("TDX_PERSISTENT_CUS") == want, s
    for s, want in (("12", 12), ("21", 21), ("11", 11), ("22", 22), ("13", 22), ("3", 22), ("1", 22), ("2", 22), ("121", 22)):
        monkeypatch.setenv("TDX_ATTN_BWD_TW", s)
        assert L.switch("TDX_ATTN_BWD_TW") == want, s
    for n, word in WORDS.items():
        for s, want in ((word, 1), ("1", 1), ("0", 0), (word[0], 0), (word.upper(), 0), (word + "x", 0), ("mfma", 0), ("auto", 0)):
            monkeypatch.setenv(n, s)
            assert L.switch(n) == want, (n, s)
    for n in set(L.switch_names()) - set(WORDS):  # a word is a value of its own row only
        monkeypatch.setenv(n, "direct")
        assert L.switch(n) == L.switch_default(n), n


def test_formerly_frozen_switches_are_read_per_call(L, monkeypatch):
    """TDX_CONV3_SMALL was read once per process (as were TDX_WGRAD_SMALL and the weight gradient's TDX_CONV3_PERM): setting
    it in a running process did nothing.  The route query is pure host code; a host buffer stands in for the arena, as in
    test_conv3_routing_is_pinned."""
    monkeypatch.delenv("TDX_CONV_IMPL", raising=False)
    lib = L.load()
    fake = ctypes.create_string_buffer(256)  # zeroed; never dereferenced by the query
    shape = (512, 0, 512, 6, 12, 4, 3)

    def kernel():
        return L.query("tdx_conv3_fwd_kernel", *shape, L.BF16, L.CONV_AUTO)

    try:
        assert lib.tdx_set_scratch(ctypes.addressof(fake), 96 << 20) == 0
        assert kernel() == L.KERNEL_SMALL
        monkeypatch.setenv("TDX_CONV3_SMALL", "0")
        assert kernel() == L.KERNEL_BRICK
        monkeypatch.delenv("TDX_CONV3_SMALL")
        assert kernel() == L.KERNEL_SMALL
        monkeypatch.setenv("TDX_CONV3_SMALL_ROWS", "0")  # "set" takes the deep forwards' own gate away as well
        assert kernel() == L.KERNEL_BRICK
        monkeypatch.setenv("TDX_CONV3_SMALL_ROWS", "many")  # an ignored value is not "set"
        assert kernel() == L.KERNEL_SMALL
    finally:
        lib.tdx_set_scratch(None, 0)
        L._ACTIVE = None  # a later GPU test in this process binds its real arena again


def test_conv1_queries_follow_the_switches_between_two_calls(L, monkeypatch):
    """TDX_CONV1_IMPL has ONE reader, conv1_route, asked per call by the forward, the fused tail and the weight gradient's plan;
    TDX_DETERMINISTIC and the arena's size are read by that plan per call: the same queries again after each change."""
    uses = [(f.name, n) for f in sorted(CSRC.glob("tdx_conv*")) if (n := len(re.findall(r"\bSW_CONV1_IMPL\b", f.read_text())))]
    assert uses == [("tdx_conv1.hip", 1)], uses
    lib = L.load()
    fake = ctypes.create_string_buffer(256)  # never dereferenced: the plan looks at the claimed size only
    fwd = lambda: L.conv1_fwd_plan(64, 64, 64, 64, 0, True, False, L.BF16)["kernel"]
    tail = lambda: L.conv1_fwd_plan(64, 64, 64, 64, 0, True, True, L.BF16)["status"]
    wgrad = lambda: L.conv1_bwd_weight_plan(32, 32, 2305, 0, L.BF16)  # one tile, ten 256-row chunks
    try:
        assert lib.tdx_set_scratch(ctypes.addressof(fake), 96 << 20) == 0
        for value, kernel, status in ((None, "h16", 0), ("direct", "vector", -2), ("0", "h16", 0), ("1", "vector", -2), (None, "h16", 0)):
            monkeypatch.delenv("TDX_CONV1_IMPL", raising=False) if value is None else monkeypatch.setenv("TDX_CONV1_IMPL", value)
            assert (fwd(), tail(), wgrad()["kernel"]) == (kernel, status, kernel), value
        for value, nslab in ((None, 0), ("1", 10), ("0", 0), ("1", 10)):
            monkeypatch.delenv("TDX_DETERMINISTIC", raising=False) if value is None else monkeypatch.setenv("TDX_DETERMINISTIC", value)
            assert (wgrad()["nsplit"], wgrad()["nslab"]) == (10, nslab), value
        assert lib.tdx_set_scratch(ctypes.addressof(fake), 256 + 4 * 1088 * 3) == 0  # room for three slabs of 32 * 32 + 32 floats, rounded up to 64
        assert (wgrad()["nsplit"], wgrad()["nslab"]) == (3, 3)
        assert lib.tdx_set_scratch(None, 0) == 0
        assert (wgrad()["nsplit"], wgrad()["nslab"]) == (1, 0)
    finally:
        lib.tdx_set_scratch(None, 0)
        L._ACTIVE = None  # a later GPU test in this process binds its real arena again


# (B, N, H) on both sides of every threshold of the attention plan.  nblk = B H ceil(N / 256), ntile = ceil(N / 64).
ATTN_SHAPES = [
    (2, 8, 4), (2, 127, 4), (2, 128, 4), (2, 144, 4),    # vector / matrix core at N = 128
    (2, 448, 4), (2, 449, 4),                             # ntile 7 / 8: norm bound
    (64, 1000, 4), (257, 1000, 1),                        # B H = 256 / 257: norm bound (nblk 1024, 1028)
    (32, 1000, 4), (27, 4700, 1), (64, 1000, 4),          # nblk 512 / 513 / 1024: stream-K only at 513
    (33, 960, 4), (33, 961, 4), (33, 1000, 4),            # nblk 528 at ntile 15 / 16 / 16: stream-K
    (1, 96 * 32 * 24, 4),                                 # BASELINE configs[4]: 1152 blocks
]


def test_attn_plan_follows_switches_and_arena_between_two_calls(L, monkeypatch):
    """attn_plan (csrc/tdx_attention.hip) is the ONE reader of the four TDX_ATTN_* switches and the one place that asks for the
    arena's size; the entry points and tdx_attn_plan ask it per call.  The library's answer against the Python restatement
    (attention_cases.expected_plan) on both sides of every threshold, for every dtype, switch setting and arena size -- the same
    queries again after each change.  A host buffer stands in for the arena: the plan looks at the claimed size only."""
    import attention_cases as A

    for sw in ("IMPL", "STREAMK", "BOUND", "BWD_TW"):
        uses = [(f.name, n) for f in sorted(CSRC.glob("tdx_attention*")) if (n := len(re.findall(rf"\bSW_ATTN_{sw}\b", f.read_text())))]
        assert uses == [("tdx_attention.hip", 1)], (sw, uses)
    lib = L.load()
    fake = ctypes.create_string_buffer(256)
    arenas = (0, A.ARENA_ZERO + A.ARENA_KMAX - 1, A.ARENA_ZERO + A.ARENA_KMAX, A.ARENA_STREAMK - 1, A.ARENA_STREAMK, 96 << 20)
    envs = [{}, {"TDX_ATTN_IMPL": "vector"}, {"TDX_ATTN_IMPL": "1"}, {"TDX_ATTN_STREAMK": "0"}, {"TDX_ATTN_BOUND": "0"},
            {"TDX_ATTN_STREAMK": "0", "TDX_ATTN_BOUND": "0"}] + [{"TDX_ATTN_BWD_TW": tw} for tw in ("11", "12", "21", "22")] + [{}]
    seen = set()
    try:
        for arena in arenas:
            assert lib.tdx_set_scratch(ctypes.addressof(fake) if arena else None, arena) == 0
            for env in envs:
                for k in A.PLAN_ENV:
                    monkeypatch.delenv(k, raising=False) if k not in env else monkeypatch.setenv(k, env[k])
                for B, N, H in ATTN_SHAPES:
                    for dt in (L.F32, L.BF16, L.F16):
                        got, want = L.attn_plan(B, N, H, 32, dt), A.expected_plan(B, N, H, 32, dt, env, arena)
                        assert got == want, (arena, env, B, N, H, dt)
                        assert L.query("tdx_attn_bwd_workspace_bytes", B, N, H, 32) == 4 * B * N * H == got["workspace"]
                        seen.add((got["fwd"], got["streamk"], got["bound"], got["tw_dq"], got["tw_dkv"]))
        # every outcome was met, and the numbers of the smallest shape that engages stream-K (tests/attention_bits_cases.py)
        assert {s[:3] for s in seen} == {("vector", 0, 0), ("mfma", 0, 0), ("mfma", 0, 1), ("mfma", 1, 0), ("mfma", 1, 1)}
        assert {s[3:] for s in seen} == {(0, 0), (1, 1), (1, 2), (2, 1), (2, 2)}
        p = L.attn_plan(33, 1000, 4, 32, L.BF16)  # the last arena and environment: 96 MB, defaults
        assert (p["nqb"], p["ntile"], p["nwg"], p["chunk"], p["streamk"], p["bound"]) == (4, 16, 512, 17, 1, 1)
        assert lib.tdx_set_scratch(ctypes.addressof(fake), A.ARENA_STREAMK - 1) == 0  # the silent fall-back, now reported
        p = L.attn_plan(33, 1000, 4, 32, L.BF16)
        assert (p["nwg"], p["chunk"], p["streamk"], p["bound"]) == (528, 16, 0, 1)
    finally:
        lib.tdx_set_scratch(None, 0)
        L._ACTIVE = None  # a later GPU test in this process binds its real arena again


def test_attn_plan_statuses(L):
    """The statuses of tdx_attn_fwd / tdx_attn_bwd before they launch anything, from the plan: D != 32 is TDX_ESHAPE (before
    the dtype is looked at), a dtype code that is no tensor format TDX_EDTYPE, a non-positive size or no plan TDX_EINVAL; the
    plan array is zeroed unless the status is TDX_OK."""
    import attention_cases as A

    for D in (16, 31, 33, 64):
        for dt in (L.F32, L.BF16, L.F16, 2, 7):
            assert L.attn_plan(2, 144, 4, D, dt) == A.expected_plan(2, 144, 4, D, dt) and L.attn_plan(2, 144, 4, D, dt)["status"] == -2
    for dt in (2, 4, -1):
        assert L.attn_plan(2, 144, 4, 32, dt) == A.expected_plan(2, 144, 4, 32, dt) and L.attn_plan(2, 144, 4, 32, dt)["status"] == -3
    for B, N, H in ((0, 144, 4), (2, 0, 4), (2, 144, 0), (-1, 144, 4)):
        assert L.attn_plan(B, N, H, 32, L.BF16)["status"] == -1
    assert L.load().tdx_attn_plan(2, 144, 4, 32, L.BF16, None) == -1


def test_python_and_library_agree_on_deterministic(L, monkeypatch):
    assert L.deterministic() is False
    for s, want in (("", False), ("0", False), ("1", True), ("2", False), ("off", False)):
        monkeypatch.setenv("TDX_DETERMINISTIC", s)
        assert L.deterministic() == (L.switch("TDX_DETERMINISTIC") != 0) == want, s


def _table_names(text):
    """Backticked TDX_... names in the rows of INTEGRATION.md's switch tables (section 5), and {name: default} of the
    library-switch table's first two columns."""
    section = text.split("## 5. Switches", 1)[1]
    rows = [l for l in section.splitlines() if l.startswith("|") and not l.startswith("|---")]
    names = set(re.findall(r"`(TDX_[A-Z0-9_]+)", "\n".join(rows)))
    lib_rows = {}
    for l in rows:
        m = re.match(r"\| `(TDX_[A-Z0-9_]+)` \| `(-?\d+)` \|", l)
        if m and "library switch" in section.split(l, 1)[0]:
            lib_rows[m.group(1)] = int(m.group(2))
    return names, lib_rows


def test_single_read_site_and_documented_table(L):
    readers = []
    for f in sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.h"))):
        if any(re.search(r"\bgetenv\s*\(", line.split("//")[0]) for line in f.read_text().splitlines()):
            readers.append(f.name)
    assert readers == ["tdx_ordered.hip"], readers

    names, lib_rows = _table_names((ROOT / "INTEGRATION.md").read_text())
    table = {n: L.switch_default(n) for n in L.switch_names()}
    assert lib_rows == table, "INTEGRATION.md's library-switch table: one row per switch of the library, with its default"
    python_side = "\n".join(f.read_text() for f in sorted((ROOT / "generative-turbulence_amd" / "turbdiff_amd").glob("*.py"))
                            + [ROOT / "bench.py"] + sorted((ROOT / "tools").rglob("*.py")) + sorted((ROOT / "tools").rglob("*.sh")))
    for n in sorted(names - set(table)):
        assert re.search(rf"\b{n}\b", python_side), f"{n}: in INTEGRATION.md's table, but neither a library switch nor read by the Python side"
