"""Development aid: compare two disassemblies made by tools/dbg/extract_isa.py function by function (python tools/dbg/cmp_isa.py A.s B.s).
Addresses and encodings are dropped; the literal of an `s_add_u32` / `s_addc_u32 sN, sN, LITERAL` (the PC-relative distance behind an
`s_getpc_b64`, which moves when code is added to the object) is normalised.  Prints the counts, the symbols on one side only and the
functions that differ with their first differing lines."""
import re, sys, hashlib
def load(p):
    fns, cur = {}, None
    for line in open(p):
        m = re.match(r'^[0-9a-f]+ <(.+)>:', line)
        if m:
            cur = m.group(1); fns[cur] = []; continue
        if cur is None or not line.strip(): continue
        ins = line.split('//')[0].strip()
        ins = re.sub(r'^(s_addc?_u32 s\d+, s\d+, )(0x[0-9a-f]+|-?\d+)$', r'\1PCREL', ins)
        if ins: fns[cur].append(ins)
    return fns
a, b = load(sys.argv[1]), load(sys.argv[2])
same = [k for k in a if k in b and a[k] == b[k]]
diff = [k for k in a if k in b and a[k] != b[k]]
print("parent functions", len(a), "new", len(b), "identical", len(same), "different", len(diff))
print("only in new:", sorted(set(b) - set(a)))
print("only in parent:", sorted(set(a) - set(b)))
for k in diff:
    la, lb = a[k], b[k]
    nd = sum(x != y for x, y in zip(la, lb)) + abs(len(la) - len(lb))
    ex = [(x, y) for x, y in zip(la, lb) if x != y][:3]
    print(k[:100], len(la), len(lb), "differing lines", nd, ex)
