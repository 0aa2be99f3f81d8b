"""The plain-text log the ez_seg functions leave behind (``ark.segmentation.ez_seg.ez_seg_utils.log_creator``): one
``name: value`` line per entry, values formatted by ``str``."""
import pathlib


def log_creator(variables_to_log: dict, base_dir: str, log_name: str = "config_values.txt"):
    """Writes the entries of ``variables_to_log`` to ``base_dir/log_name``, replacing the file, and says where."""
    target = pathlib.Path(base_dir, log_name)
    target.write_text("".join("%s: %s\n" % item for item in variables_to_log.items()))
    print("Values saved to %s" % target)
