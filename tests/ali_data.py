"""The blocks `smalt map -a` prints behind the line of a mapped alignment, read back from a program's output: shared by the fixture
generator (tests/golden/make_golden_ali.py), which records per fixture how often each corner of the layout occurs, and the tests,
which look for the same counts in the committed text before they compare anything with it."""
import re

WIDTH = 60                  # alignment columns per line (DEFAULT_LINWIDTH_ALI, report.c:50)
MARKS = (("gap", "-"), ("transition", "i"), ("transversion", "v"), ("unknown", "?"), ("nonstandard", "!"))


def blocks_of(text):
    """output of a program (bytes) -> [(q_first, read row, q_last, marker row, s_first, reference row, s_last)]"""
    lines = text.decode().split("\n")
    out = []
    for i, ln in enumerate(lines):
        if not ln.startswith("    QUERY: "):
            continue
        q = re.match(r"^ {4}QUERY: ([ \d-]{10}) (.*) (-?\d+) *$", ln)
        s = re.match(r"^REFERENCE: ([ \d-]{10}) (.*) (-?\d+) *$", lines[i + 2])
        assert q and s and lines[i + 1].startswith(" " * 22) and lines[i + 3] == "" and lines[i + 4] == "", (i, ln)
        mark = lines[i + 1][22:]
        assert len(q.group(2)) == len(mark) == len(s.group(2)) <= WIDTH, (i, ln)
        out.append((int(q.group(1)), q.group(2), int(q.group(3)), mark, int(s.group(1)), s.group(2), int(s.group(3))))
    return out


def shapes_of(text):
    """counts of the corners of the layout in a program's output (manifest_ali.json: "shapes")"""
    bl = blocks_of(text)
    sh = dict(blocks=len(bl), empty_blocks=sum(1 for b in bl if not b[3]), full_lines=sum(1 for b in bl if len(b[3]) == WIDTH),
              descending=sum(1 for b in bl if b[1] and b[0] > b[2]), gap_in_last_column=sum(1 for b in bl if len(b[3]) == WIDTH and b[3][-1] == "-"))
    for name, ch in MARKS:
        sh[name] = sum(b[3].count(ch) for b in bl)
    return sh
