"""Print the shading census (oracle_py.EVENT_NAMES) as a markdown table: event x scene, the number of pixels whose
samples produced the event, for the catalogue scenes at the parity tests' 64 x 36 x 4 spp and for the aimed scenes of
tests/shading_scenes.py at 48 x 32 x 8 spp.  CPU only (the oracle).  * marks an event the scene owns.

    python tools/shading_census.py > table.md
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "raytracing-potato_amd"), os.path.join(REPO, "tests")]


def table(columns):
    from oracle import oracle_py as O
    names = [c[0] for c in columns]
    print("| event | " + " | ".join(names) + " |")
    print("|---|" + "---:|" * len(names))
    for e in O.EVENT_NAMES:
        print(f"| {e} | " + " | ".join(f"{c[1][e]}{'*' if e in c[2] else ''}" if c[1][e] else "." for c in columns)
              + " |")
    print()


def main():
    import shading_scenes as S
    import test_shading_census as T
    cat = []
    for n in S.CATALOGUE_FRAMES:
        sc, p = S.catalogue(n)
        cat.append((n, S.event_pixels(S.census(sc, p)[2]), T.CATALOGUE_OWNS.get(n, [])))
    print("Catalogue scenes, 64 x 36 x 4 spp (2,304 pixels):\n")
    table(cat)
    aimed = [(n, S.event_pixels(S.census(S.scene(n), S.params(n))[2]), S.OWNS[n]) for n in S.SCENES]
    print("Aimed scenes, 48 x 32 x 8 spp (1,536 pixels):\n")
    table(aimed)


if __name__ == "__main__":
    main()
