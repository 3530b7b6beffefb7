# Run on a machine with the GPU: tools/side_stats_profile.py <form> (blocking | batch) under rocprofv3 --kernel-trace --stats, the kernel table into
# <directory>/<form>_kernel_stats.txt (usage: profile_side_stats.sh <form> [directory], default profile_out/side) (two passes of the form per run: halve the calls and totals for one 64-picture 4K batch).  For the table
# of a build without the batched form, name it in SVT_PRODUCT_LIB and ask for `blocking`.
FORM=${1:-batch}
export TMPDIR=/tmp
O=${2:-profile_out/side}
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_$FORM -- python tools/side_stats_profile.py $FORM > $O/$FORM.json 2> $O/$FORM.err < /dev/null || { echo "profiled run failed"; tail -5 $O/$FORM.err; exit 1; }
DB=$(find $O/prof_$FORM -name "*.db" | head -1)
if [ -n "$DB" ]; then
  python profiles/summarize_rocpd.py $DB "tools/side_stats_profile.py $FORM (64 4K pictures, the form run twice) under rocprofv3 --kernel-trace --stats" > $O/${FORM}_kernel_stats.txt
  head -14 $O/${FORM}_kernel_stats.txt
else
  echo "no rocpd database"; tail -5 $O/$FORM.err; exit 1
fi
rm -rf $O/prof_$FORM
