"""The engine handle's device memory, pinned words, streams and events have ONE owner (bbai_engine.hip: ResKind / Scoped / Owner).  The raw
HIP calls that make or release such a resource occur only between the two marker comments that bracket those helpers: every other line of
the file goes through them, so bbai_destroy never has to name a buffer."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = os.path.join(ROOT, "babyai_amd", "csrc", "bbai_engine.hip")
BEGIN, END = "// ---- owner helpers: begin", "// ---- owner helpers: end"
RAW = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree|hipStreamCreate\w*|hipStreamDestroy|hipEventCreate\w*|hipEventDestroy)\b")


def strip_comments(text):
    """C++ source without its comments and with its string / character literals emptied; line breaks stay (line numbers survive)."""
    out, i, n = [], 0, len(text)
    while i < n:
        two = text[i:i + 2]
        if two == "//":
            while i < n and text[i] != "\n":
                i += 1
        elif two == "/*":
            end = text.find("*/", i + 2)
            end = n if end < 0 else end + 2
            out.append("\n" * text.count("\n", i, end))
            i = end
        elif text[i] in "\"'":
            q = text[i]
            i += 1
            while i < n and text[i] != q:
                i += 2 if text[i] == "\\" else 1
            i += 1
            out.append(q + q)
        else:
            out.append(text[i])
            i += 1
    return "".join(out)


def raw_calls(code):
    return [(code.count("\n", 0, m.start()) + 1, m.group(1)) for m in RAW.finditer(code)]


def test_strip_comments_keeps_code_and_drops_prose():
    src = 'a = hipMalloc(&p, 8);  // hipFree(p) later\n/* hipEventCreate\n hipStreamDestroy */ b = "hipFree"; c = \'"\'; hipFree(p);\n'
    assert raw_calls(strip_comments(src)) == [(1, "hipMalloc"), (3, "hipFree")]


def test_raw_resource_calls_only_inside_the_owner_helpers():
    with open(ENGINE) as f:
        text = f.read()
    assert text.count(BEGIN) == 1 and text.count(END) == 1, "one pair of marker comments"
    lo = text.count("\n", 0, text.index(BEGIN)) + 1
    hi = text.count("\n", 0, text.index(END)) + 1
    assert lo < hi
    calls = raw_calls(strip_comments(text))
    outside = [(line, name) for line, name in calls if not lo < line < hi]
    assert not outside, "raw resource calls outside the owner helpers: %r" % (outside,)
    inside = {name for line, name in calls if lo < line < hi}
    # (the helpers are where they all live: a file that lost them to another place would pass the check above vacuously)
    assert {"hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipStreamDestroy", "hipEventDestroy"} <= inside
    assert any(c.startswith("hipStreamCreate") for c in inside) and any(c.startswith("hipEventCreate") for c in inside)
