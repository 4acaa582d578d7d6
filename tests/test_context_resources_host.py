"""The context's resources without a GPU, read from the source of the library (tardis_amd/csrc/tardis_mc_hip.hip): every device buffer,
event and stream that TardisMcContext or a struct nested in it declares is named by that struct's release(), tardis_mc_destroy frees
nothing by hand, and hipFree is called by DevBuf alone -- so that a resource someone adds cannot be forgotten silently."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESOURCE = re.compile(r"^(?:DevBuf|hipEvent_t|hipStream_t|std::vector<hipEvent_t>)\s+(.*)$", re.S)


def _source():
    text = open(os.path.join(ROOT, "tardis_amd", "csrc", "tardis_mc_hip.hip")).read()
    return re.sub(r"//[^\n]*", "", text)  # (no string of the file holds a "//")


def _block(text, open_brace):
    """text[open_brace] is a '{': the index of the '}' that closes it."""
    depth = 0
    for i in range(open_brace, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return i
    raise AssertionError("unbalanced braces")


def _function_body(text, signature):
    at = text.index(signature)
    open_brace = text.index("{", at)
    return text[open_brace + 1:_block(text, open_brace)]


def _structs(name, body, out):
    """out[name] = (resource members of the struct itself, the body of its release() or None); nested structs likewise, under
    'Outer::Inner'.  Bodies of nested structs and of member functions are cut out before the members are read."""
    own, release = "", None
    i = 0
    while i < len(body):
        if body[i] != "{":
            own += body[i]
            i += 1
            continue
        close = _block(body, i)
        head = own[max(own.rfind(";"), own.rfind("}")) + 1:].strip()  # what stands in front of this '{' since the last statement
        nested = re.match(r"struct\s*(\w*)$", head)
        if nested:
            tail = re.match(r"\s*(\w+)\s*;", body[close + 1:])
            _structs(f"{name}::{nested.group(1) or tail.group(1)}", body[i + 1:close], out)
            own = own[:own.rfind(head)]
            i = close + 1 + (tail.end() if tail else 0)
            continue
        if re.search(r"\bvoid release\(\)$", head):
            release = body[i + 1:close]
            own = own[:own.rstrip().rfind("void release()")]
        elif re.search(r"\)\s*(const)?$", head):  # another member function: its locals are no members
            own = own[:own.rfind(head)]
        else:                                      # a brace initialiser
            own += "{}"
        i = close + 1
    members = []
    for statement in own.split(";"):
        m = RESOURCE.match(statement.strip())
        if m:
            for declarator in re.sub(r"=\s*\{\}", "", m.group(1)).split(","):
                members.append(re.match(r"\s*(\w+)", declarator).group(1))
    out[name] = (members, release)


def _context_structs():
    src = _source()
    at = src.index("struct TardisMcContext {")
    open_brace = src.index("{", at)
    out = {}
    _structs("TardisMcContext", src[open_brace + 1:_block(src, open_brace)], out)
    return out


def test_the_parser_sees_the_structs_and_their_members():
    structs = _context_structs()
    assert len(structs) >= 15 and "TardisMcContext::OpacityUpdate" in structs and "TardisMcContext::EventLog" in structs
    top, _ = structs["TardisMcContext"]
    assert "stream" in top and "ev_start" in top and "ev_chunk" in top and "staging" in top
    assert "ev_rows" not in top  # (a nested struct's members are its own)
    assert structs["TardisMcContext::OpacityUpdate"][0][-1] == "ev" and "n_t" in structs["TardisMcContext::OpacityUpdate"][0]
    assert {"li_f64", "li_i64", "li_rec"} <= set(structs["TardisMcContext::Packets"][0])  # arrays and scalars of one declaration
    assert sum(len(members) for members, _ in structs.values()) > 150


def test_every_resource_is_named_by_the_release_of_its_struct():
    missing = []
    for name, (members, release) in _context_structs().items():
        for member in members:
            if release is None or not re.search(rf"\b{member}\b", release):
                missing.append(f"{name}::{member}")
    assert not missing, "not released by their struct: " + ", ".join(missing)


def test_destroy_frees_nothing_by_hand():
    body = _function_body(_source(), "void tardis_mc_destroy(TardisMcContext *ctx)")
    assert body.count("release()") >= 15
    for word in (r"\.p\b", "hipFree", "hipEventDestroy", "hipStreamDestroy", "hipHostFree"):
        assert not re.search(word, body), word


def test_only_the_buffer_type_calls_hipfree():
    src = _source()
    at = src.index("struct DevBuf {")
    open_brace = src.index("{", at)
    rest = src[:at] + src[_block(src, open_brace) + 1:]
    assert "hipFree" in src[at:_block(src, open_brace)] and "hipFree" not in rest
