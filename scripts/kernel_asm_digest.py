"""Device code of HIP sources, function by function, as hashes: for refactors that must leave every kernel as it was.
  hipcc $(CXXFLAGS) --cuda-device-only -S fft_tile.hip -o new/fft_tile.s        (the Makefile's CXXFLAGS; once per source and tree)
  python scripts/kernel_asm_digest.py digest new/*.s > new.json
  python scripts/kernel_asm_digest.py compare parent.json new.json
A block is a function from `<symbol>:` to its `.Lfunc_end`, with its `.amdhsa_kernel ... .end_amdhsa_kernel` descriptor.  The
`__hip_cuid_` lines are dropped and the per-file function index in local labels and loop comments (`.LBB<n>_`, `BB<n>_`,
`.Lfunc_begin<n>`, `.Lfunc_end<n>`) is replaced, with the blanks that pad a comment to its column, so that a function that moved inside a file, or to another one, hashes the same.
`digest` prints {"blocks": {symbol: sha256}, "all": sha256 of the blocks concatenated in symbol order}; `compare` lists the
symbols on one side only and the ones whose blocks differ, and exits 1 if any block differs."""
import hashlib, json, re, sys

START = re.compile(r"^([A-Za-z_$][\w$.]*):\s*; @")
END = re.compile(r"^\.Lfunc_end\d+:")
INDEX = re.compile(r"(\.LBB|BB|\.Lfunc_begin|\.Lfunc_end)\d+")
PAD = re.compile(r"[ \t]+;")            # a label's comment is padded to a fixed column: one space more or less with a 2-digit index


def blocks_of(text):
    out, name, lines, desc = {}, None, [], {}
    kernel = None
    for line in text.splitlines():
        if "__hip_cuid_" in line:
            continue
        if name is None:
            m = START.match(line)
            if m:
                name, lines = m.group(1), []
        if name is not None:
            lines.append(PAD.sub(" ;", INDEX.sub(r"\1", line)))
            if END.match(line):
                out[name] = lines
                name = None
            continue
        if line.strip().startswith(".amdhsa_kernel "):           # a descriptor outside its function's block
            kernel = line.split()[1]
            desc[kernel] = []
        if kernel is not None:
            desc[kernel].append(line)
            if line.strip() == ".end_amdhsa_kernel":
                kernel = None
    for k, d in desc.items():
        out[k] = out.get(k, []) + d
    return {k: "\n".join(v) + "\n" for k, v in out.items()}


def digest(paths):
    blocks = {}
    for p in paths:
        for k, v in blocks_of(open(p).read()).items():
            # (a kernel of a shared header is compiled into every file that uses it)
            assert blocks.setdefault(k, v) == v, f"{k}: two files hold different code under this name"
    whole = hashlib.sha256("".join(blocks[k] for k in sorted(blocks)).encode()).hexdigest()
    return {"blocks": {k: hashlib.sha256(v.encode()).hexdigest() for k, v in sorted(blocks.items())}, "all": whole}


def compare(a, b):
    a, b = (json.load(open(p))["blocks"] for p in (a, b))
    for k in sorted(set(a) - set(b)): print("only in the first: ", k)
    for k in sorted(set(b) - set(a)): print("only in the second:", k)
    changed = [k for k in sorted(set(a) & set(b)) if a[k] != b[k]]
    for k in changed: print("differs:           ", k)
    print(f"{len(set(a) & set(b)) - len(changed)} of {len(set(a) & set(b))} common blocks identical")
    return 1 if changed else 0


if __name__ == "__main__":
    if sys.argv[1] == "digest":
        print(json.dumps(digest(sys.argv[2:]), indent=1))
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
