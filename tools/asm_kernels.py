"""Parser of the gfx950 assembly of the library's device code (hipcc -S --cuda-device-only), shared by count_valu.sh and
compare_device_asm.sh: the text is split at the kernels' `_ZN3fhe...:` labels."""
import re


def kernels(path):
    """{kernel symbol: (body, descriptor)}: the instruction lines from the label to s_endpgm and the lines of the kernel's
    .amdhsa_kernel block, comments dropped.  Basic-block labels carry the function's ordinal in the file (.LBB<n>_<k>): it is
    dropped too, so that a kernel compares equal wherever in the file it was emitted."""
    cur, desc, out = None, None, {}
    for line in open(path):
        m = re.match(r'^(_ZN3fhe\S+):', line)
        if m:
            cur = m.group(1)
            out[cur] = ([], [])
            continue
        t = re.sub(r'\.LBB\d+_', '.LBB_', line.split(';')[0].strip())
        m = re.match(r'^\.amdhsa_kernel\s+(\S+)', t)
        if m:
            desc = m.group(1)
        elif t == '.end_amdhsa_kernel':
            desc = None
        elif desc in out and t:
            out[desc][1].append(t)
        elif cur and t:
            out[cur][0].append(t)
            if t == 's_endpgm':
                cur = None
    return out


def opcodes(body):
    """the instruction mnemonics of a kernel body (labels and directives left out)"""
    return [t.split()[0] for t in body if not t.startswith('.') and not t.endswith(':')]
