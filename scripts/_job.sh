cd $GRAFT_REPO_ROOT
out=${1:?usage: bash scripts/_job.sh <output directory>}
mkdir -p "$out"
python bench.py --full > "$out"/bench.json 2> "$out"/bench.err
tail -c 300 "$out"/bench.json
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
