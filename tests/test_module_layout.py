"""The package's host-side layout: ``predict`` and ``data`` keep every public name they ever had
(the same objects as in the kernel-family modules the definitions live in), and the modules import
each other at module level only, without a cycle.  No GPU."""
import ast
import os

PKG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "prostate-cancer-multimodal-segmentation_amd")

# one module per kernel family (csrc/<name>.hip) plus what they share
FAMILIES = ["_args", "nifti", "geometry", "resample", "intensity", "window", "components", "distance", "lesions",
            "align"]
LAYERED = FAMILIES + ["data", "predict", "utils.metrics"]

# the functions, classes and constants predict.py and data.py defined before the split
PREDICT_NAMES = """
MODALITIES load_multimodal_images normalise intensity_window normalise_window Normalisation DEFAULT_LEVELS
joint_histogram normalised_mutual_information Alignment register_rigid joint_histogram_device
register_rigid_device register_case register_case_device register_dataset prepare_case tta_mean mask_on_grid
MAX_KEEP_LARGEST label_components filter_components fill_holes postprocess postprocess_device
label_components_device TABLE_CAPACITY component_table overlap_pairs match_lesions lesion_table lesion_metrics
component_table_device overlap_pairs_device lesion_table_device lesion_metrics_device surface edt_sq
distance_transform surface_metrics surface_device distance_transform_device surface_metrics_device
MAX_WINDOW_AXIS window_starts window_grid window_weights gather_windows blend_windows sliding_window_predict
gather_windows_device blend_windows_device sliding_window_device prepare_case_device CasePrediction
preprocess_image ModelPredictor
""".split()
DATA_NAMES = """
DEFAULT_MODALITIES read_nifti_header read_nifti RawVolume read_nifti_raw read_nifti_geometry write_nifti resample
resample_affine MAX_CONTROL_POINTS field_displacement resample_deform Augment compose_transform volume_affine
world_matrix RIGID_NAMES rigid_world world_centre rigid_correction align_affine compose_affine case_affine
affine12_of registration_fixed Transform draw_transform MAX_PATCHES MAX_PATCH_AXIS PatchSampling resample_patch
draw_patches pick_origins resample_device is_raw_batch assemble_batch assemble_patch_batch device_batch
ProstateDataset get_dataloader BatchShard kfold_indices get_kfold_splits
""".split()


def _tree(module):
    with open(os.path.join(PKG_DIR, *module.split(".")) + ".py") as f:
        return ast.parse(f.read())


def _defined(module):
    """The names a module's own top-level statements define (imports excluded)."""
    names = set()
    for node in _tree(module).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            names.add(node.name)
        elif isinstance(node, ast.Assign):
            names.update(t.id for t in node.targets if isinstance(t, ast.Name))
    return names


def test_predict_and_data_keep_their_public_names():
    import importlib

    import pcms_amd  # noqa: F401
    assert len(PREDICT_NAMES) == 57 and len(DATA_NAMES) == 43
    families = {m: (importlib.import_module("pcms_amd." + m), _defined(m)) for m in FAMILIES}
    for owner, names in (("predict", PREDICT_NAMES), ("data", DATA_NAMES)):
        mod, own = importlib.import_module("pcms_amd." + owner), _defined(owner)
        for name in names:
            obj = getattr(mod, name)  # resolves
            homes = [m for m, (_, defined) in families.items() if name in defined]
            assert (name in own) != bool(homes) and len(homes) <= 1, (owner, name, homes)
            for m in homes:  # a re-export is the family module's own object
                assert getattr(families[m][0], name) is obj, (owner, name, m)


def _imports(module, node):
    """The LAYERED modules a relative import statement names, seen from ``module``."""
    if not isinstance(node, ast.ImportFrom) or node.level == 0:
        return []
    base = module.split(".")[:-1]
    base = base[:len(base) - (node.level - 1)]
    if node.module:
        found = [".".join(base + [node.module])]
    else:
        found = [".".join(base + [a.name]) for a in node.names]
    return [m for m in found if m in LAYERED]


def test_layered_modules_import_each_other_at_module_level_without_a_cycle():
    graph = {}
    for module in LAYERED:
        tree = _tree(module)
        graph[module] = sorted({m for node in tree.body for m in _imports(module, node)})
        for fn in ast.walk(tree):
            if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
                lazy = [m for node in ast.walk(fn) for m in _imports(module, node)]
                assert not lazy, f"{module}.{getattr(fn, 'name', 'lambda')} imports {lazy} inside its body"
    assert graph["data"] and graph["predict"] and graph["utils.metrics"] and "predict" not in graph["data"]
    done, path = set(), []

    def visit(m):
        assert m not in path, "import cycle: " + " -> ".join(path[path.index(m):] + [m])
        if m in done:
            return
        path.append(m)
        for dep in graph[m]:
            visit(dep)
        path.pop()
        done.add(m)

    for module in LAYERED:
        visit(module)
