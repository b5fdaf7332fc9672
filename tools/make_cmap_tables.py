#!/usr/bin/env python3
"""Writes sais_amd/_cmap_tables.py: the byte tables of matplotlib's `inferno` and `viridis` colormaps, for installations without
matplotlib (sais_amd.attnviz.colormap_lut prefers matplotlib's own table when it is importable; tests/test_attnviz_host.py holds
the bundled copy to it).  The data are matplotlib's (matplotlib/_cm_listed.py, CC0): 256 RGB rows each, as
Colormap.__call__(bytes=True) uses them, (lut * 255) truncated to uint8.

    python tools/make_cmap_tables.py
"""
import os
import textwrap

import numpy as np
from matplotlib import colormaps

NAMES = ("inferno", "viridis")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sais_amd", "_cmap_tables.py")


def table(name):
    cmap = colormaps[name]
    if not cmap._isinit:
        cmap._init()
    assert cmap.N == 256
    return (cmap._lut[:256, :3] * 255).astype(np.uint8)


if __name__ == "__main__":
    with open(OUT, "w") as fh:
        fh.write('"""Byte tables [256, 3] of matplotlib colormaps as hex strings (R, G, B per row).  Written by '
                 'tools/make_cmap_tables.py: do not edit."""\n')
        fh.write("HEX = {\n")
        for name in NAMES:
            body = "\n".join(f'        "{line}"' for line in textwrap.wrap(table(name).tobytes().hex(), 96))
            fh.write(f'    "{name}": (\n{body}),\n')
        fh.write("}\n")
    print("wrote", os.path.normpath(OUT))
