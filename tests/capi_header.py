"""include/*.h read as data for tests/test_capi_binding.py: DFM_API declarations with their parameters, descriptor
structs field by field, integer constants.  A regex reader of these headers' plain C, not a C parser: what it cannot
read raises, and the test counts the DFM_API and struct tokens, so nothing is skipped in silence."""
import glob
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(INCLUDE, '*.h')))      # a new header is found
INT = r'-?(?:0[xX][0-9a-fA-F]+|[1-9]\d*|0)'


def strip_comments(text):
    """/* */ and // comments blanked; line breaks stay, so a line of code is still a line"""
    text = re.sub(r'/\*.*?\*/', lambda m: ' ' + '\n' * m.group().count('\n'), text, flags=re.S)
    return re.sub(r'//[^\n]*', ' ', text)


def code(header):
    with open(os.path.join(INCLUDE, header)) as f:
        return strip_comments(f.read())


def parameter(text):
    """'const float *cam2img' -> ('cam2img', 'float', 1): name, C type without const, pointer depth (a [] counts)"""
    m = re.fullmatch(r'([\w\s*]+?)\b(\w+)\s*((?:\[[^\]]*\]\s*)*)', text.strip())
    if not m:
        raise ValueError(f'cannot read the parameter {text!r}')
    ctype = ' '.join(w for w in m.group(1).replace('*', ' ').split() if w != 'const')
    return m.group(2), ctype, m.group(1).count('*') + m.group(3).count('[')


def declarations(code):
    """{name: (return type, [parameter(...), ...])} of every DFM_API function that starts a line, in order"""
    decls = {}
    for m in re.finditer(r'^[ \t]*DFM_API\s+([\w\s\*]+?)\b(dfm_\w+)\s*\(', code, flags=re.M):
        i, depth, cuts = m.end(), 1, [m.end() - 1]
        while depth:                                             # to the closing parenthesis, nested ones skipped
            depth += (code[i] == '(') - (code[i] == ')')
            if depth == 0 or (depth == 1 and code[i] == ','):
                cuts.append(i)
            i += 1
        if not code[i:].lstrip().startswith(';'):
            raise ValueError(f'{m.group(2)}: no ; after the parameter list')
        params = [code[a + 1:b].strip() for a, b in zip(cuts, cuts[1:])]
        params = [] if params in ([''], ['void']) else [parameter(p) for p in params]
        decls[m.group(2)] = (' '.join(m.group(1).split()), params)
    return decls


def constants(code):
    """{name: value} of every ``#define DFM_NAME <integer>`` and every enumerator given an explicit integer"""
    found = re.findall(rf'^[ \t]*#[ \t]*define[ \t]+(DFM_\w+)[ \t]+({INT})[ \t]*$', code, flags=re.M)
    for body in re.findall(r'\benum\s+\w*\s*\{(.*?)\}', code, flags=re.S):
        found += re.findall(rf'(?:^|,)\s*(DFM_\w+)\s*=\s*({INT})\s*(?=,|$)', body)
    return {name: int(value, 0) for name, value in found}


def structs(code, known):
    """{struct: [(field, C type, array length or None), ...]} of every ``typedef struct dfm_x { ... } dfm_x;``.  An
    array length is an integer expression over the constants ``known``: offset[DFM_VOXEL_MAX_BATCH + 1]"""
    out = {}
    for name, body in re.findall(r'\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;', code, flags=re.S):
        out[name] = []
        for line in filter(None, (' '.join(s.split()) for s in body.split(';'))):
            ctype, items = re.fullmatch(r'((?:\w+ )+)(.+)', line).groups()
            for item in items.split(','):                       # 'int32_t h_in, w_in': one type, several names
                field, length = re.fullmatch(r'\s*(\w+)\s*(?:\[([\w\s+\-*()]+)\])?\s*', item).groups()
                out[name].append((field, ctype.strip(), length and eval(length, {'__builtins__': {}}, dict(known))))
    return out
