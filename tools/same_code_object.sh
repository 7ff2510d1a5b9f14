#!/bin/bash
# Is the device code object of this tree the same bytes as at another revision?  No GPU needed.
#   bash tools/same_code_object.sh [rev] [flag set ...]        rev defaults to HEAD; a flag set is ONE argument ("plain" = no -D)
# For each flag set: both trees (rev by git archive, and the working tree) compiled device-only with kernel_regs.sh's hipcc line
# plus -cuid=mdstep, then cmp.  One line per flag set: "identical", or "DIFFERS old new" (the two objects, kept).  Exit 1 if any
# flag set differs.  It reports identity only; it looks at nothing inside the objects.
# A flag set that differs is compiled once more per tree and a match between any old / new pair accepted ("identical (2nd
# compile)"): -DMD_STAMP compiles to one of several objects from one source, its three device globals (g_stamp_buf, g_env_order,
# g_contacts_buf) take their places in .bss in any order.  Still no match: the code (.text), the kernel descriptors (.rodata) and
# the metadata (.note) of the two code objects compared byte for byte: "same .text .rodata .note, symbol values differ".  That
# is a WEAKER claim than "identical" (the symbol tables, .bss layout and dynamic section are not compared) and also exits 0.  It
# says more than a disassembly with the globals' addresses masked would: the kernels reach a global through the GOT, whose
# entries are filled at load time by symbol index, so no address stands in .text and every byte of it is compared.  Seen with
# -DMD_STAMP: whole objects differing in 4 to 6 bytes, all of them symbol values in .dynsym / .symtab.
# $HIPCC and $JOBS (compiles at a time, 16 at the most) are honoured.
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
LLVM=${LLVM:-/opt/rocm/lib/llvm/bin}
JOBS=${JOBS:-$(nproc)}
[ "$JOBS" -gt 16 ] && JOBS=16
REV=${1:-HEAD}
[ $# -gt 0 ] && shift
if [ $# -eq 0 ]; then
    set -- plain -DMD_STAMP -DMD_ENV_SKIP=1 -DMD_SC_SKIP=1 -DMD_TD_SKIP=1 -DMD_ENV_BLOCK=128 -DMD_WAVE_ENVS=1 \
        -DMD_LOC_ROAD_FIRST=0 -DMD_OBS_LOCKSTEP=0 -DMD_OBS_AHEAD=0 -DMD_CONTACTS_FLAT=0 -DMD_TRIGGER_EARLY=0 -DMD_NT_STAGE=0 -DMD_LEAN_VIEW=0 -DMD_WRITE_BACK_OWN=0
fi
SETS=("$@")

TMP=$(mktemp -d /tmp/same_code_object.XXXXXX)
mkdir "$TMP/old" "$TMP/obj"
git -C "$ROOT" archive "$REV" | tar -x -C "$TMP/old" || { echo "cannot export $REV"; exit 2; }

# compile <tree> <flag set index> <object>: the flags of kernel_regs.sh, from inside the tree so that both see the same paths
compile() {
    local flags=${SETS[$2]}
    [ "$flags" = plain ] && flags=
    # shellcheck disable=SC2086
    (cd "$1" && $HIPCC -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -Iinclude $flags -cuid=mdstep --cuda-device-only \
        -c metadrive_ped_amd/csrc/mdstep.hip -o "$3") 2> "$3.log" || echo "compile failed: $3.log" >&2
}
# run the queued "tree index object" lines, $JOBS at a time
run_queue() {
    local n=0 tree i obj
    while read -r tree i obj; do
        compile "$tree" "$i" "$obj" &
        n=$((n + 1))
        [ "$n" -ge "$JOBS" ] && { wait -n; n=$((n - 1)); }
    done
    wait
}
same() { [ -s "$1" ] && [ -s "$2" ] && cmp -s "$1" "$2"; }
# the sections of the code object that hold no symbol value, as a hex dump
sections() {
    "$LLVM/clang-offload-bundler" --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$1" --output="$1.co" --unbundle &&
        "$LLVM/llvm-objdump" -s -j .text -j .rodata -j .note "$1.co" | grep -v 'file format' > "$1.s"
}

for i in "${!SETS[@]}"; do
    echo "$TMP/old $i $TMP/obj/$i.old.o"
    echo "$ROOT $i $TMP/obj/$i.new.o"
done > "$TMP/queue"
run_queue < "$TMP/queue"

again=()
for i in "${!SETS[@]}"; do
    same "$TMP/obj/$i.old.o" "$TMP/obj/$i.new.o" || again+=("$i")
done
for i in ${again[@]+"${again[@]}"}; do
    echo "$TMP/old $i $TMP/obj/$i.old2.o"
    echo "$ROOT $i $TMP/obj/$i.new2.o"
done > "$TMP/queue"
run_queue < "$TMP/queue"

status=0
for i in "${!SETS[@]}"; do
    o=$TMP/obj/$i.old n=$TMP/obj/$i.new
    if same "$o.o" "$n.o"; then
        verdict=identical
    elif same "$o.o" "$n"2.o || same "$o"2.o "$n.o" || same "$o"2.o "$n"2.o; then
        verdict="identical (2nd compile)"
    elif sections "$o.o" && sections "$n.o" && [ -s "$o.o.s" ] && cmp -s "$o.o.s" "$n.o.s"; then
        verdict="same .text .rodata .note, symbol values differ"
    else
        verdict="DIFFERS $o.o $n.o"
        status=1
    fi
    printf '%-24s %s\n' "${SETS[$i]}" "$verdict"
done
if [ "$status" -eq 0 ]; then rm -rf "$TMP"; else rm -rf "$TMP/old"; fi
exit $status
