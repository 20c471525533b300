"""The launches of the C ABI, read from include/adain_hip.h: the declarations whose last parameter is ``adain_stream_t stream``.  Not a
test module.  test_far_batch_host.py and test_limits_host.py hold their hand-written tables to this list, so that an entry point added
to the header fails both until it has a row or a stated reason for having none."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "adain_hip.h")
_DECLARATION = re.compile(r"\bADAIN_API\b[^;()]*?\b(adain_\w+)\s*\(([^;()]*)\)\s*;")


def launches(text=None):
    """The names, in the header's order.  ``text``: a header's text in place of the file's."""
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    names = []
    for m in _DECLARATION.finditer(text):
        last = " ".join(m.group(2).split(",")[-1].split())
        if last == "adain_stream_t stream":
            names.append(m.group(1))
    assert len(set(names)) == len(names), "a launch is declared twice"
    return names


def audit(table_calls, exempt, what):
    """AssertionError unless every launch of the header is in exactly one of ``table_calls`` (the calls a table has rows for) and
    ``exempt`` ({call: reason}), every key of ``exempt`` is a launch of the header and every reason says something."""
    names = set(launches())
    table_calls = set(table_calls)
    missing = sorted(names - table_calls - set(exempt))
    assert not missing, f"{what}: launches of include/adain_hip.h with neither a row nor a reason: {missing}"
    both = sorted(table_calls & set(exempt))
    assert not both, f"{what}: these have a row and a reason for having none: {both}"
    gone = sorted(set(exempt) - names)
    assert not gone, f"{what}: exempted, but no launch of the header: {gone}"
    unknown = sorted(table_calls - names)
    assert not unknown, f"{what}: rows for calls the header does not declare as launches: {unknown}"
    empty = sorted(k for k, v in exempt.items() if not (isinstance(v, str) and v.strip()))
    assert not empty, f"{what}: a reason is empty: {empty}"
