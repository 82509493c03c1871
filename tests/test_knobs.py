"""The library's configuration surface is ONE file (csrc/knobs.hpp): every environment variable it honours in a shipped build is in the
`pub` list there, described in that header's comment, and mentioned in the docs a user reads; nothing else in csrc/ calls getenv."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "noble-curves_amd", "csrc")


def _read(*p):
    with open(os.path.join(*p)) as f:
        return f.read()


def test_public_knobs_are_listed_described_and_documented():
    src = _read(CSRC, "knobs.hpp")
    m = re.search(r"pub\[\]\s*=\s*\{([^}]*)\}", src)
    assert m, "the list of public knobs moved"
    pub = re.findall(r'"(NCG_[A-Z0-9_]+)"', m.group(1))
    assert len(pub) == len(set(pub)) and "NCG_LANE_QUEUES" in pub and "NCG_NO_FINISH_THREADS" in pub
    header = src.split("#pragma once")[0]
    always = header.split("A/B builds only")[0]
    docs = _read(ROOT, "INTEGRATION.md") + _read(ROOT, "DESIGN.md")
    for k in pub:
        assert k in always, "%s is honoured by the shipped library but not described under 'always honoured'" % k
    for k in ("NCG_LANE_QUEUES", "NCG_NO_FINISH_THREADS"):     # the two that change what the library does to the embedding process
        assert k in _read(ROOT, "INTEGRATION.md"), k
    for k in pub:
        assert k in docs or k in ("NCG_TIMING",), "%s is not mentioned in INTEGRATION.md / DESIGN.md" % k


def test_only_knobs_hpp_reads_the_environment():
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".hpp")) or name == "knobs.hpp":
            continue
        text = _read(CSRC, name)
        assert "getenv" not in text, "%s reads the environment directly (use ncg::knob)" % name


def _public_knobs():
    m = re.search(r"pub\[\]\s*=\s*\{([^}]*)\}", _read(CSRC, "knobs.hpp"))
    assert m, "the list of public knobs moved"
    return set(re.findall(r'"(NCG_[A-Z0-9_]+)"', m.group(1)))


def test_every_knob_read_is_public():
    """A name outside pub[] would read as a runtime choice but always return its default: a dead switch."""
    pub = _public_knobs()
    calls = 0
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".hpp")) or name == "knobs.hpp":
            continue
        text = _read(CSRC, name)
        for call in re.finditer(r"\bknob(?:_set)?\s*\(", text):
            calls += 1
            m = re.match(r'\s*"([^"]*)"', text[call.end():])
            assert m, "%s: knob call without a string literal name" % name
            assert m.group(1) in pub, "%s reads %s, which is not a public knob (knobs.hpp pub[])" % (name, m.group(1))
    assert calls >= len(pub)


def test_no_ab_build_mode():
    """The library has one build: nothing in csrc/, tools/ or the Makefile refers to the removed A/B build flag."""
    paths = [os.path.join(CSRC, n) for n in sorted(os.listdir(CSRC))]
    tools = os.path.join(ROOT, "tools")
    paths += [os.path.join(tools, n) for n in sorted(os.listdir(tools))]
    for p in paths:
        if not os.path.isfile(p):
            continue
        with open(p, "rb") as f:
            assert b"NCG_AB_BUILD" not in f.read(), "%s mentions NCG_AB_BUILD" % os.path.relpath(p, ROOT)
