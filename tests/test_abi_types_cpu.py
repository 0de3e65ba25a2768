"""CPU: the argument types of the ctypes binding against include/e3d_hip.h.

hip.py restates every C signature by hand (``_SIGNATURES``).  The compiler holds the header to the definitions and the
other tests compare names; this one parses every ``e3d_*`` prototype of the header and requires the binding's return type
and whole argument list to be its translation: every pointer ``c_void_p`` (``const char*``: ``c_char_p``), every scalar
type its ctypes twin.  A ``uint64_t`` bound as ``c_int``, or two arguments swapped in a list of thirty, passes every other
test that happens to use small values.  Needs neither the shared library nor a GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double, "uint8_t": ctypes.c_uint8,
           "unsigned": ctypes.c_uint, "long": ctypes.c_long, "size_t": ctypes.c_size_t}
PROTOTYPE = re.compile(r"([A-Za-z_][\w\s\*]*?)\b(e3d_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))      # preprocessor lines


def ctype_of(decl, is_return=False):
    """The ctypes type of one C parameter declaration (``const float* const* grads``, ``int64_t lda``, ``void``...)."""
    decl = " ".join(decl.replace("*", " * ").split())
    if "*" in decl:
        base = decl[:decl.index("*")].split()
        return ctypes.c_char_p if base == ["const", "char"] else ctypes.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if not is_return:
        assert len(words) == 2, f"cannot read the parameter {decl!r}"        # type and name
        words = words[:1]
    assert len(words) == 1, f"cannot read the type of {decl!r}"
    if words[0] == "void":
        assert is_return
        return None
    return SCALARS[words[0]]


def parse_header(text):
    """{name: (return ctype, [argument ctypes])} of every e3d_* prototype."""
    out = {}
    for ret, name, params in PROTOTYPE.findall(strip_comments(text)):
        ret = ret.replace('extern "C"', " ").replace("{", " ").replace("}", " ")
        params = params.strip()
        args = [] if params in ("", "void") else [ctype_of(a) for a in params.split(",")]
        assert name not in out, f"{name} declared twice"
        out[name] = (ctype_of(ret, is_return=True), args)
    return out


def test_the_parser_reads_the_forms_the_header_uses():
    text = """/* int e3d_in_a_comment(int x); */
    #define E3D_X 1
    const char* e3d_a(void);   // int e3d_also_a_comment(void);
    void e3d_b(int waves, int64_t
               n);
    int64_t e3d_c(float* const* params, const float* const* grads, const uint8_t* mask, uint32_t site, uint64_t seed,
                  double d, float f, const int32_t* idx, void* stream);"""
    P = ctypes.c_void_p
    assert parse_header(text) == {
        "e3d_a": (ctypes.c_char_p, []), "e3d_b": (None, [ctypes.c_int, ctypes.c_int64]),
        "e3d_c": (ctypes.c_int64, [P, P, P, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double, ctypes.c_float, P, P])}


def test_every_binding_signature_is_the_translation_of_its_prototype(pkg):
    header = parse_header(open(os.path.join(ROOT, "include", "e3d_hip.h")).read())
    binding = pkg.hip._SIGNATURES
    assert len(header) > 100                                        # (the parser found the prototypes at all)
    assert set(header) == set(binding), (sorted(set(header) - set(binding)), sorted(set(binding) - set(header)))
    wrong = []
    for name, (ret, args) in header.items():
        b_ret, b_args = binding[name]
        if ret is not b_ret:
            wrong.append(f"{name}: returns {ret}, bound as {b_ret}")
        if len(args) != len(b_args):
            wrong.append(f"{name}: {len(args)} arguments, bound with {len(b_args)}")
            continue
        wrong += [f"{name}: argument {i} is {a.__name__}, bound as {getattr(b, '__name__', b)}"
                  for i, (a, b) in enumerate(zip(args, b_args)) if a is not b]
    assert not wrong, "\n".join(wrong)
