"""INTEGRATION.md section 6 and the switches the library reads say the same thing.

The names are taken from the sources as text: every UPSIDE_HIP_* name inside a string literal of upside-md_amd/csrc/ is a switch
the library reads, except the ones listed in warn_removed_switches() (engine.cpp), which it only warns about."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'upside-md_amd', 'csrc')
NAME = re.compile(r'UPSIDE_HIP_[A-Z0-9_]+')
LITERAL = re.compile(r'"((?:[^"\\\n]|\\.)*)"')


def _sources():
    out = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith(('.cpp', '.hip', '.h')):
            with open(os.path.join(CSRC, fn)) as f:
                out[fn] = f.read()
    return out


def _literal_names(text):
    return {n for lit in LITERAL.findall(text) for n in NAME.findall(lit)}


def _removed_list(sources):
    """(names, text of the initialiser list) of warn_removed_switches()"""
    src = sources['engine.cpp']
    body = src[src.index('static void warn_removed_switches()'):]
    lst = re.search(r'for \(const char\* v : \{(.*?)\}\)', body, re.S).group(0)
    return _literal_names(lst), lst


def _section6():
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
        doc = f.read()
    sec = doc[doc.index('## 6. Environment switches'):]
    nxt = re.search(r'^## ', sec[3:], re.M)
    return doc, (sec[:nxt.start() + 3] if nxt else sec)


def test_switches_read_and_switches_documented_agree():
    sources = _sources()
    removed, removed_text = _removed_list(sources)
    assert len(removed) >= 16 and 'UPSIDE_HIP_BP_SPLIT' in removed and 'UPSIDE_HIP_SCHEDULE' in removed
    read = set().union(*(_literal_names(t) for t in sources.values())) - removed
    assert len(read) > 40, sorted(read)

    doc, sec6 = _section6()
    documented = set(NAME.findall(doc))
    assert not read - documented, 'read by csrc/, missing from INTEGRATION.md: %s' % sorted(read - documented)

    rows = [ln for ln in sec6.splitlines() if ln.startswith('|')]
    assert len(rows) > 30
    in_rows = {n for ln in rows for n in NAME.findall(ln)}
    assert not in_rows - read, 'in the table of section 6, not read by csrc/: %s' % sorted(in_rows - read)

    paragraph = [p for p in sec6.split('\n\n') if 'removed the switches' in p]
    assert len(paragraph) == 1
    ticked = set(re.findall(r'`([A-Z0-9_]+)`', paragraph[0]))
    for name in sorted(removed):
        assert name in ticked or name[len('UPSIDE_HIP_'):] in ticked, '%s is not named in the "removed" paragraph of section 6' % name
        for fn, text in sources.items():
            rest = text.replace(removed_text, '') if fn == 'engine.cpp' else text
            assert not re.search(name + r'(?![A-Z0-9_])', rest), '%s is removed but still named in csrc/%s' % (name, fn)
