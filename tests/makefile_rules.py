"""What the host tests ask of csrc/Makefile, in one place: a source built with the exact-arithmetic flags is in EXACT_SRC, the
static pattern rule over the EXACT_SRC objects compiles with $(COMMON) $(EXACT), and no other rule can build that object.  The
Makefile's own text is read (as much of make's syntax as it uses: `:=` lists, $(wildcard ..), $(VAR:%.a=%.b), static pattern
rules); nothing is compiled."""
import fnmatch
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, '3d-sdn_amd', 'csrc')
EXACT_RULE = '$(EXACT_OBJS): ../lib/obj/%.o: %.hip $(HDRS) | ../lib/obj'
EXACT_RECIPE = '\t$(HIPCC) $(COMMON) $(EXACT) -c $< -o $@'


def _logical_lines(text):
    """comment lines dropped, backslash continuations joined: a list may be wrapped"""
    lines, at = [], ''
    for raw in text.splitlines():
        if raw.startswith('#'):
            continue
        if raw.endswith('\\'):
            at += raw[:-1] + ' '
            continue
        lines.append(at + raw)
        at = ''
    return lines


def _expand(text, variables):
    def one(m):
        body = m.group(1)
        if body.startswith('wildcard '):
            return ' '.join(sorted(os.path.basename(p) for pat in body.split()[1:] for p in glob.glob(os.path.join(CSRC, pat))))
        subst = re.fullmatch(r'(\w+):%(\S*)=(\S*)%(\S*)', body)
        if subst:
            name, old, pre, new = subst.groups()
            words = _expand(variables[name], variables).split()
            assert all(w.endswith(old) for w in words), (name, old)
            return ' '.join(pre + w[:len(w) - len(old)] + new for w in words)
        return _expand(variables[body], variables)
    return re.sub(r'\$\(([^()]*)\)', one, text)


def parse(text):
    """the variables, and the rules as (target words, the rule's line, its recipe lines)"""
    variables, rules = {}, []
    for line in _logical_lines(text):
        assign = re.match(r'^(\w+)\s*[:?]?=\s*(.*)$', line)
        if assign:
            variables[assign.group(1)] = assign.group(2).strip()
        elif line.startswith('\t'):
            rules[-1][2].append(line)
        elif ':' in line:
            rules.append((_expand(line.split(':')[0], variables).split(), line, []))
    return variables, rules


def _can_build(target, obj):
    return fnmatch.fnmatchcase(obj, target.replace('%', '*')) if '%' in target else target == obj


def assert_built_exactly(source, text=None):
    """`source` (X.hip) is in EXACT_SRC and only the EXACT rule builds ../lib/obj/X.o"""
    text = open(os.path.join(CSRC, 'Makefile')).read() if text is None else text
    variables, rules = parse(text)
    assert source in variables['EXACT_SRC'].split(), '%s is not in EXACT_SRC' % source
    obj = '../lib/obj/' + source[:-len('.hip')] + '.o'
    builders = [(line, recipe) for targets, line, recipe in rules if any(_can_build(t, obj) for t in targets)]
    assert builders == [(EXACT_RULE, [EXACT_RECIPE])], (obj, builders)
