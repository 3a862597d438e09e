"""The one reader of include/panst3r_hip.h for the host tests: prototypes, struct fields and integer #defines as the header declares them.

Types are normalised to what the ABI distinguishes: `const` and parameter names are dropped and every pointer is written 'T*' ('void*', 'float*',
'pst_gemm_params*', 'char*').  The header is plain C with one declarator style, so a few regular expressions read all of it; `prototypes()` asserts
that nothing that looks like a declaration was left unparsed."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'panst3r_hip.h')
SCALARS = ('int', 'int32_t', 'int64_t', 'uint64_t', 'float', 'double')
_IDENT = r'[A-Za-z_][A-Za-z0-9_]*'
_STRUCT = re.compile(r'typedef struct (%s) \{(.*?)\} \1;' % _IDENT, flags=re.S)


def _code():
    """the header without comments"""
    with open(HEADER) as f:
        return re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)


def _type(words):
    t = ' '.join(w for w in words.replace('*', ' * ').split() if w != 'const')
    return t.replace(' *', '*')


def _declarator(decl):
    """'const float* x' -> ('float*', 'x', None);  'float c2w[12]' -> ('float', 'c2w', 12)"""
    m = re.fullmatch(r'(.*?)(%s)\s*(?:\[(\d+)\])?' % _IDENT, decl.strip(), flags=re.S)
    assert m and m.group(1).strip(), 'cannot read the declaration %r' % decl
    return _type(m.group(1)), m.group(2), int(m.group(3)) if m.group(3) else None


def defines():
    """{name: value} of the integer #defines"""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define (%s)\s+(-?\d+)\s*$' % _IDENT, _code(), flags=re.M)}


def structs():
    """{struct name: [(field name, type, array length or None)]} in declaration order"""
    out = {}
    for name, body in _STRUCT.findall(_code()):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(';'))):
            first, *more = decl.split(',')                      # 'int32_t M, N, K': the declarators after the first share its type
            typ, fname, n = _declarator(first)
            fields.append((fname, typ, n))
            for d in more:
                assert re.fullmatch(_IDENT, d.strip()), 'cannot read the declarator %r of %s' % (d, name)
                fields.append((d.strip(), typ, None))
        out[name] = fields
    return out


def prototypes():
    """[(function name, return type, [parameter types])] in declaration order"""
    text = _STRUCT.sub('', _code())
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    text = re.sub(r'extern "C" \{|^\}\s*$', '', text, flags=re.M)
    out = []
    for decl in filter(None, (d.strip() for d in text.split(';'))):
        m = re.fullmatch(r'(.*?)\b(pst_[a-z0-9_]+)\s*\((.*)\)', decl, flags=re.S)
        assert m, 'cannot read the declaration %r' % decl
        params = [] if m.group(3).strip() == 'void' else [_declarator(p)[0] for p in m.group(3).split(',')]
        out.append((m.group(2), _type(m.group(1)), params))
    assert len({p[0] for p in out}) == len(out)
    return out
