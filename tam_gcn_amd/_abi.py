"""Parser of include/tamgcn.h, the one declaration of the C ABI: every struct field and every parameter of every entry point
with base type, pointer, `const` (`const T*` = read, `T*` = write) and array count, every return type and every integer
#define.  Pure Python, no ctypes: _lib.py derives the binding from what this returns, the audits under tests/ classify the
pointers with it.  Anything the parser does not understand raises ValueError; there is no branch that guesses."""
import os
import re

HEADER = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'tamgcn.h'))

BASE_TYPES = ('unsigned char', 'long long', 'unsigned', 'int', 'float', 'double', 'void', 'char')


class Decl:
    """One field, parameter or return type (name '').  kind: 'scalar' | 'r' | 'w' (device or host array read / written) |
    'stream' | 'struct' (by value) | 'desc' (pointer to a struct of the header)."""
    __slots__ = ('name', 'base', 'ptr', 'const', 'count', 'kind')

    def __init__(self, name, base, ptr, const, count, structs):
        self.name, self.base, self.ptr, self.const, self.count = name, base, ptr, const, count
        if not ptr:
            self.kind = 'struct' if base in structs else 'scalar'
        elif base in structs:
            self.kind = 'desc'
        elif base == 'void' and name == 'stream' and not const:
            self.kind = 'stream'
        else:
            self.kind = 'r' if const else 'w'

    def __repr__(self):
        return f'<{self.kind} {"const " if self.const else ""}{self.base}{"*" if self.ptr else ""} {self.name}' \
               f'{"[%d]" % self.count if self.count else ""}>'


def _parse_decl(text, structs, defines):
    """'const float* w[TAMGCN_TCONV_MAXB]' / 'int N, K' -> [Decl]."""
    s = ' '.join(text.split())
    const = s.startswith('const ')
    if const:
        s = s[6:]
    base = None
    for t in sorted(tuple(BASE_TYPES) + tuple(structs), key=len, reverse=True):
        if s == t or s.startswith(t + ' ') or s.startswith(t + '*'):
            base, s = t, s[len(t):].strip()
            break
    if base is None:
        raise ValueError(f'tamgcn.h: unknown type in {text!r}')
    ptr = s.startswith('*')
    if ptr:
        s = s[1:].strip()
        if '*' in s:
            raise ValueError(f'tamgcn.h: pointer to pointer in {text!r}')
    out = []
    for nm in [p.strip() for p in s.split(',')] if s else ['']:
        m = re.fullmatch(r'(\w*)(?:\[(\w+)\])?', nm)
        if not m:
            raise ValueError(f'tamgcn.h: cannot parse {text!r}')
        cnt = m.group(2)
        if cnt is not None:
            cnt = int(cnt) if cnt.isdigit() else defines[cnt]
        out.append(Decl(m.group(1), base, ptr, const, cnt, structs))
    if ptr and len(out) != 1:
        raise ValueError(f'tamgcn.h: several names behind one pointer type in {text!r}')
    return out


def parse_abi(path=HEADER):
    """(structs, funcs, rets, defines): {struct name: [Decl]}, {entry point: [Decl]} (a `void` parameter list is []),
    {entry point: Decl of its return type} and {name: value} of the integer #defines."""
    with open(path) as f:
        text = f.read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$', text, re.M)}
    text = re.sub(r'^[ \t]*#[^\n]*$', ' ', text, flags=re.M)
    text = text.replace('extern "C" {', ' ')
    structs = {}
    pat = re.compile(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;', re.S)
    for m in pat.finditer(text):                           # names first: a struct may hold another by value
        if m.group(1) != m.group(3):
            raise ValueError(f'tamgcn.h: struct {m.group(1)} is typedef-ed as {m.group(3)}')
        structs[m.group(1)] = None
    for m in pat.finditer(text):
        fields = []
        for stmt in m.group(2).split(';'):
            if stmt.strip():
                fields += _parse_decl(stmt, structs, defines)
        structs[m.group(1)] = fields
    rest = pat.sub(';', text)
    funcs, rets = {}, {}
    for stmt in rest.split(';'):
        s = ' '.join(stmt.split())
        if s in ('', '}'):
            continue
        m = re.fullmatch(r'(.+?)\b(tamgcn_\w+) ?\((.*)\)', s)
        if not m:
            raise ValueError(f'tamgcn.h: statement not understood: {s[:80]!r}')
        params = []
        if m.group(3).strip() != 'void':
            for p in m.group(3).split(','):
                params += _parse_decl(p, structs, defines)
        funcs[m.group(2)] = params
        rets[m.group(2)], = _parse_decl(m.group(1), structs, defines)
    return structs, funcs, rets, defines


def parse_header(path=HEADER):
    """(structs, funcs) of parse_abi(): what the audits need."""
    return parse_abi(path)[:2]
