'use strict'
/**
 * @hocuspocus/extension-gpu-merge -- drop-in persistence extension whose
 * merge / diff / state-vector work runs on MI355X.
 *
 * Mirrors the reference's persistence contract:
 *   interface Extension            packages/server/src/types.ts:36-63
 *   DatabaseConfiguration{fetch,store}  packages/extension-database/src/Database.ts:10-20
 *   storePayload.state: Buffer     packages/server/src/types.ts:329-331
 *
 * What changes versus extension-database: instead of Y.encodeStateAsUpdate(doc)
 * on every debounced store (Database.ts:55-60), the state is computed in a GPU
 * batch with every other document whose store fires in the same window:
 * Y.mergeUpdates([base, ...updates since base]), then (normalize, the default)
 * the doc-normalized snapshot of that merge -- Y.encodeStateAsUpdate(
 * Y.applyUpdate(new Y.Doc(yDocOptions), merged)), the bytes extension-database
 * stores for a fresh load of the same updates, with the document's own gc
 * option.  With normalize: false the stored bytes are the bare merge.  Either
 * is a valid V1 update of the same document state, byte-identical to yjs;
 * loading applies it exactly as Database.ts:44-50 does.
 */
const { GpuEngine, GpuEnginePool, fnv1a64, YgmError } = require('./engine')
const { SyncResponder } = require('./sync')
const { RedisFanout } = require('./redis')
const { UpdateLog } = require('./log')

/**
 * A batched document store.  `fromDatabase` adapts any DatabaseConfiguration
 * (sqlite / s3 / custom) document by document.
 */
class DocumentStore {
  /** @returns {Promise<(Uint8Array|Uint8Array[]|null)[]>} */
  async fetchMany (payloads) { return payloads.map(() => null) }
  /** @param {{payload: any, state: Buffer}[]} entries */
  async storeMany (entries) {}

  static fromDatabase (config) {
    const s = new DocumentStore()
    s.fetchMany = payloads => Promise.all(payloads.map(p => config.fetch ? config.fetch(p) : null))
    s.storeMany = entries => Promise.all(entries.map(e => config.store ? config.store({ ...e.payload, state: e.state }) : undefined))
    return s
  }
}

class GpuMerge {
  /**
   * @param {{store?: DocumentStore|Function, fetch?: Function, device?: number, Y?: any,
   *          engine?: GpuEngine, batchWindowMs?: number, maxBatchDocs?: number, compat135?: boolean, floats?: boolean,
   *          onRefused?: 'reference'|'throw', normalize?: boolean, normalizeMaxBytes?: number,
   *          gc?: 'document'|boolean}} configuration
   *   gc ('document' by default): whether the normalized snapshot and the responder's / fan-out's replies are
   *   garbage-collected.  The reference passes yDocOptions { gc, gcFilter } (types.ts:152-154; per document from
   *   onCreateDocument, Hocuspocus.ts:331-344) to the Y.Doc constructor, and a gc: false document stores and sends its
   *   deleted Items with their content (Database.ts:55-60).  'document' reads `document.gc` of the live document this
   *   extension captures (afterLoadDocument, onStoreDocument); true / false force one behaviour for every document.
   *   A custom gcFilter (a JavaScript predicate per Item) cannot be reproduced: such deployments use normalize: false.
   *   onRefused: what a store does when the engine refuses ONE document (a per-document status: content
   *   yjs would re-encode, ENONCANON; a corrupt stored base, EMALFORMED / ERANGE / ESURROGATE / EDEPTH) --
   *   'reference' (default): store Y.encodeStateAsUpdate(document) like extension-database and record it in
   *   `refused`; 'throw': reject the store.  A failed batch (EDEVICE, ENOMEM, EINVAL, an addon or driver
   *   error) always rejects the store (Hocuspocus logs and rethrows, Hocuspocus.ts:431-435): the product has
   *   no CPU fallback for a lost or failing GPU (SURVEY.md §5)
   *   normalize (default true): store the doc-normalized snapshot of the merge, Y.encodeStateAsUpdate(
   *   Y.applyUpdate(new Y.Doc(), merged)) computed on the GPU (SURVEY.md §8f-1) -- deleted content
   *   garbage-collected and adjacent structs merged, the bytes extension-database stores for a fresh load of
   *   the same updates (Database.ts:55-60); a document outside the snapshot kernel's envelope keeps its merged
   *   bytes (`unnormalized`).  normalize: false stores the bare Y.mergeUpdates bytes.
   *   normalizeMaxBytes (default 32768): merged states larger than this are stored as the bare merge (counted in
   *   `sizeSkipped`): the snapshot kernel runs a document on ONE GPU thread (yjs's integration is a serial chain),
   *   3-5 us per byte, and a batch takes its largest document's time: ~0.1-0.15 s at the limit, seconds for the ~1 MB
   *   documents of BASELINE config C5, whose merge takes milliseconds (DESIGN.md 6.R6, tools/snap_probe.py).  Both
   *   forms load identically.
   */
  constructor (configuration = {}) {
    this.extensionName = 'GpuMerge'
    // after Redis (priority 1000, which takes the store lock first), before plain storage extensions (100)
    this.priority = configuration.priority || 900
    this.configuration = configuration
    this.normalize = configuration.normalize !== false
    this.gc = configuration.gc === undefined ? 'document' : configuration.gc
    if (this.gc !== 'document' && this.gc !== true && this.gc !== false) throw new TypeError("GpuMerge: gc is 'document', true or false")
    this.normalizeMaxBytes = configuration.normalizeMaxBytes === undefined ? 32768 : configuration.normalizeMaxBytes
    /** stores whose merged state was over normalizeMaxBytes (kept as the bare merge) */
    this.sizeSkipped = 0
    // drop-in for `new Database({ fetch, store })`, or a batched DocumentStore instance
    const st = configuration.store
    this.store = st && typeof st.storeMany === 'function'
      ? st
      : DocumentStore.fromDatabase({ fetch: configuration.fetch, store: typeof st === 'function' ? st : undefined })
    this.Y = configuration.Y || null
    this.engine = configuration.engine || null
    /** documentName -> { base: Uint8Array|null, log: UpdateLog (packed captured updates), doc?: Y.Doc, onUpdate?: Function,
     *  gc?: boolean (the live document's gc option, as last seen) } */
    this.docs = new Map()
    /** stores that fell back to Y.encodeStateAsUpdate(document) because the engine refused the merge */
    this.refused = []
    /** normalize: stores that kept the merged bytes (snapshot outside the kernel's envelope) */
    this.unnormalized = []
    /** jsonOf / versionJson / sharedJsonOf / versionSharedJson: documents whose JSON the engine refused (outside ygm_json_v1's envelope: the caller keeps
     *  its yjs path, transformer.fromYdoc, for them) */
    this.unserialized = []
  }

  _Y () { if (!this.Y) this.Y = require('yjs'); return this.Y }
  _engine () {
    if (!this.engine) {
      const c = this.configuration
      const opts = { device: c.device || 0, compat135: c.compat135, floats: c.floats, batchWindowMs: c.batchWindowMs, maxBatchDocs: c.maxBatchDocs }
      // several GPUs of the node: documents sharded by fnv1a64(documentName) mod N (SURVEY.md §8e)
      this.engine = c.devices && c.devices.length > 1 ? new GpuEnginePool({ ...opts, devices: c.devices }) : new GpuEngine(opts)
    }
    return this.engine
  }

  /**
   * A batched SyncStep1 responder over this extension's captured state (stored snapshot + the
   * updates since): reconnect storms answered by one GPU diff batch (SURVEY.md §8f-2, src/sync.js).
   */
  syncResponder () {
    return new SyncResponder({
      engine: this._engine(),
      getState: async name => { const e = this.docs.get(name); return e ? (e.base ? [e.base] : []).concat(e.log.toArray()) : null },
      getDocOptions: name => ({ gc: this._gcOf(name) })
    })
  }

  // is the named document garbage-collected?  The configured value, or ('document') the live document's own option
  // as captured at load / store; a document never seen is collected, the Y.Doc default
  _gcOf (documentName, document) {
    if (this.gc !== 'document') return this.gc
    const e = this.docs.get(documentName)
    if (document && typeof document.gc === 'boolean') { if (e) e.gc = document.gc; return document.gc }
    return e && typeof e.gc === 'boolean' ? e.gc : true
  }

  /** Batched extension-redis fan-out over the same captured state (SURVEY.md §8f-3, src/redis.js) */
  redisFanout ({ publish, identifier, prefix, windowMs }) {
    const r = this.syncResponder()
    return new RedisFanout({ engine: this._engine(), getState: r.getState, getDocOptions: r.getDocOptions, publish, identifier, prefix, windowMs })
  }

  // the named documents' current states: base and log merged as the responder merges them (one merge batch for those
  // with a log); null for a document that is not loaded
  async _statesOf (names) {
    const eng = this._engine()
    const parts = names.map(n => { const e = this.docs.get(n); return e ? (e.base ? [e.base] : []).concat(e.log.toArray()) : null })
    const multi = parts.map((p, i) => p && p.length > 1 ? i : -1).filter(i => i >= 0)
    const merged = !multi.length ? [] : typeof eng.shardOf === 'function'
      ? await eng.mergeMany(multi.map(i => names[i]), multi.map(i => parts[i])) : await eng.mergeMany(multi.map(i => parts[i]))
    const out = parts.map(p => !p ? null : p.length === 1 ? p[0] : p.length === 0 ? Uint8Array.from([0, 0]) : null)
    multi.forEach((i, k) => { out[i] = merged[k] })
    return out
  }

  /**
   * Version history (INTEGRATION.md "Version history").  takeVersions(names): one version -- yjs's encoded snapshot,
   * Y.encodeSnapshot(Y.snapshot(doc)) -- per loaded document, in one GPU batch over the captured states (base and log
   * merged as the responder merges them) -> Map name -> Uint8Array; a document that is not loaded, or whose state
   * the engine refuses, is left out of the map.
   */
  async takeVersions (names) {
    const eng = this._engine()
    const states = await this._statesOf(names)
    const idx = names.map((_, i) => i).filter(i => states[i] && !(states[i] instanceof Error))
    const pooled = typeof eng.shardOf === 'function'
    const res = !idx.length ? [] : pooled ? await eng.takeVersionMany(idx.map(i => names[i]), idx.map(i => states[i])) : await eng.takeVersionMany(idx.map(i => states[i]))
    const out = new Map()
    idx.forEach((i, k) => { if (!(res[k] instanceof Error)) out.set(names[i], new Uint8Array(res[k])) })
    return out
  }

  /**
   * restoreVersions([{ documentName, version, gc }]): per entry the update of the document as it was at `version`,
   * Y.encodeStateAsUpdate(Y.createDocFromSnapshot(doc, Y.decodeSnapshot(version), new Y.Doc({ gc }))) (gc default
   * true), in one GPU batch.  Returns one settled result per entry, { status: 'fulfilled', value } or { status:
   * 'rejected', reason }: a document that resolves to gc: true is rejected with yjs's own "originDoc must not be
   * garbage collected", one that is not loaded or that the engine refuses with that error -- each without
   * disturbing the other entries.  There is no CPU path.  With an engine that has restoreVersionShared the entries are
   * grouped by document (stable within a document) and each document's state goes up, and is snapshotted, once for
   * all of its versions; the results return in the caller's entry order either way.
   */
  async restoreVersions (entries) {
    const eng = this._engine()
    const out = new Array(entries.length)
    const live = []
    entries.forEach((e, i) => {
      if (!this.docs.has(e.documentName)) out[i] = { status: 'rejected', reason: new Error('GpuMerge: document ' + e.documentName + ' is not loaded') }
      else if (this._gcOf(e.documentName) !== false) out[i] = { status: 'rejected', reason: new Error('originDoc must not be garbage collected') }
      else live.push(i)
    })
    if (live.length) {
      const names = Array.from(new Set(live.map(i => entries[i].documentName)))
      const states = await this._statesOf(names)
      const stateOf = i => states[names.indexOf(entries[i].documentName)]
      const ok = live.filter(i => { const s = stateOf(i); if (s instanceof Error || !s) { out[i] = { status: 'rejected', reason: s || new Error('no state') }; return false } return true })
      const settle = (i, r) => { out[i] = r instanceof Error ? { status: 'rejected', reason: r } : { status: 'fulfilled', value: new Uint8Array(r) } }
      const pooled = typeof eng.shardOf === 'function'
      if (ok.length && typeof eng.restoreVersionShared === 'function') {
        const docs = Array.from(new Set(ok.map(i => entries[i].documentName)))   // the admitted documents, first seen first
        const at = new Map(docs.map((n, k) => [n, k]))
        const order = ok.slice().sort((x, y) => at.get(entries[x].documentName) - at.get(entries[y].documentName) || x - y)
        const sts = docs.map(n => states[names.indexOf(n)])
        const askState = order.map(i => at.get(entries[i].documentName))
        const versions = order.map(i => entries[i].version)
        const opts = order.map(i => entries[i].gc === false ? 1 : 0)
        const res = pooled ? await eng.restoreVersionShared(docs, sts, askState, versions, opts) : await eng.restoreVersionShared(sts, askState, versions, opts)
        order.forEach((i, k) => settle(i, res[k]))
        return out
      }
      const opts = ok.map(i => entries[i].gc === false ? 1 : 0)
      const res = !ok.length ? [] : pooled
        ? await eng.restoreVersionMany(ok.map(i => entries[i].documentName), ok.map(stateOf), ok.map(i => entries[i].version), opts)
        : await eng.restoreVersionMany(ok.map(stateOf), ok.map(i => entries[i].version), opts)
      ok.forEach((i, k) => settle(i, res[k]))
    }
    return out
  }

  /**
   * Plain text (INTEGRATION.md "Text of a document / of a version").  textOf(names, { field, deep }): what each loaded
   * document says, in one GPU batch over the captured states (base and log merged as takeVersions merges them) ->
   * Map name -> string.  deep: false is doc.getText(field).toString(); deep: true (the default: Tiptap documents keep
   * their text in XmlText nodes under the XmlFragment `field`) also descends into nested types, one '\n' after each
   * unless the text is still empty or already ends in one.  A document that is not loaded, or whose state the engine
   * refuses, is left out of the map.
   */
  async textOf (names, { field = 'default', deep = true } = {}) {
    const eng = this._engine()
    const states = await this._statesOf(names)
    const idx = names.map((_, i) => i).filter(i => states[i] && !(states[i] instanceof Error))
    const fields = idx.map(() => field)
    const res = !idx.length ? [] : typeof eng.shardOf === 'function'
      ? await eng.textMany(idx.map(i => names[i]), idx.map(i => states[i]), fields, { deep })
      : await eng.textMany(idx.map(i => states[i]), fields, { deep })
    const out = new Map()
    idx.forEach((i, k) => { if (!(res[k] instanceof Error)) out.set(names[i], res[k]) })
    return out
  }

  /**
   * versionTexts(entries, { field, deep }): restoreVersions(entries) followed by one text batch over the fulfilled
   * results -- a one-line preview per saved version without a Y.Doc per version.  Settled per entry as
   * restoreVersions is: { status: 'fulfilled', value: string } or { status: 'rejected', reason }.
   */
  async versionTexts (entries, { field = 'default', deep = true } = {}) {
    const eng = this._engine()
    const out = await this.restoreVersions(entries)
    const ok = out.map((r, i) => r.status === 'fulfilled' ? i : -1).filter(i => i >= 0)
    if (!ok.length) return out
    const fields = ok.map(() => field)
    const res = typeof eng.shardOf === 'function'
      ? await eng.textMany(ok.map(i => entries[i].documentName), ok.map(i => out[i].value), fields, { deep })
      : await eng.textMany(ok.map(i => out[i].value), fields, { deep })
    ok.forEach((i, k) => { out[i] = res[k] instanceof Error ? { status: 'rejected', reason: res[k] } : { status: 'fulfilled', value: res[k] } })
    return out
  }

  /**
   * Document JSON (INTEGRATION.md "Document JSON / webhook bodies").  jsonOf(names, { field, parse }): what each loaded
   * document is -- JSON.stringify(TiptapTransformer.fromYdoc(document, field)), the body the reference's webhook sends
   * -- in one GPU batch over the captured states -> Map name -> JSON string, or the parsed object with parse: true.  A
   * document that is not loaded is left out; one the engine refuses (a root that is no XmlFragment of elements and
   * texts, a float attribute, ...) is left out and named in `unserialized`: the caller keeps its yjs path for it.
   * field: a string (default 'default') is one root, fromYdoc(document, field); null or [] is every field,
   * fromYdoc(document) -- the reference webhook's call -- and an array of names is fromYdoc(document, names): both give
   * the object keyed by field, from one load of each state (ygm_json_fields_v1).
   */
  async jsonOf (names, { field = 'default', parse = false } = {}) {
    const states = await this._statesOf(names)
    const idx = names.map((_, i) => i).filter(i => states[i] && !(states[i] instanceof Error))
    const res = !idx.length ? [] : await this._jsonMany(idx.map(i => names[i]), idx.map(i => states[i]), field)
    const out = new Map()
    idx.forEach((i, k) => {
      if (res[k] instanceof Error) this.unserialized.push({ documentName: names[i], code: res[k].code || String(res[k]) })
      else out.set(names[i], parse ? JSON.parse(res[k]) : res[k])
    })
    return out
  }

  // one JSON batch over states: a string field is a root name (ygm_json_v1), null or an array a field list
  // (ygm_json_fields_v1); docNames shard the batch over a pool's engines
  _jsonMany (docNames, states, field) {
    const eng = this._engine()
    const pool = typeof eng.shardOf === 'function'
    if (typeof field === 'string') {
      const roots = states.map(() => field)
      return pool ? eng.jsonMany(docNames, states, roots) : eng.jsonMany(states, roots)
    }
    if (field !== null && !Array.isArray(field)) throw new TypeError('field: a root name, null (every field) or an array of names')
    const lists = states.map(() => field)
    return pool ? eng.jsonFieldsMany(docNames, states, lists) : eng.jsonFieldsMany(states, lists)
  }

  /**
   * versionJson(entries, { field, parse }): restoreVersions(entries) followed by one JSON batch over the fulfilled
   * results -- a saved version shown as a document, without a Y.Doc per version.  Settled per entry as restoreVersions
   * is: { status: 'fulfilled', value: string | object } or { status: 'rejected', reason } (a refused version is
   * rejected with the engine's error and named in `unserialized`).  field: as jsonOf's.
   */
  async versionJson (entries, { field = 'default', parse = false } = {}) {
    const out = await this.restoreVersions(entries)
    const ok = out.map((r, i) => r.status === 'fulfilled' ? i : -1).filter(i => i >= 0)
    if (!ok.length) return out
    const res = await this._jsonMany(ok.map(i => entries[i].documentName), ok.map(i => out[i].value), field)
    ok.forEach((i, k) => {
      if (res[k] instanceof Error) {
        this.unserialized.push({ documentName: entries[i].documentName, code: res[k].code || String(res[k]) })
        out[i] = { status: 'rejected', reason: res[k] }
      } else out[i] = { status: 'fulfilled', value: parse ? JSON.parse(res[k]) : res[k] }
    })
    return out
  }

  /**
   * toJSON of shared types that are not rich text (INTEGRATION.md "Map / Array / Text documents").
   * sharedJsonOf(names, { root, type, parse }): what each loaded document's root is --
   * JSON.stringify(document.getMap(root).toJSON()) for type 'map' (the default), getArray for 'array', getText for 'text':
   * the fromYdoc of a custom webhook transformer -- in one GPU batch over the captured states -> Map name -> JSON
   * string, or the parsed value with parse: true.  A document that is not loaded is left out; one the engine refuses
   * (a nested Xml type, binary content, a non-integer number, ...) is left out and named in `unserialized`: the caller
   * keeps its yjs path for it.
   */
  async sharedJsonOf (names, { root = 'default', type = 'map', parse = false } = {}) {
    const states = await this._statesOf(names)
    const idx = names.map((_, i) => i).filter(i => states[i] && !(states[i] instanceof Error))
    const res = !idx.length ? [] : await this._toJsonMany(idx.map(i => names[i]), idx.map(i => states[i]), root, type)
    const out = new Map()
    idx.forEach((i, k) => {
      if (res[k] instanceof Error) this.unserialized.push({ documentName: names[i], code: res[k].code || String(res[k]) })
      else out.set(names[i], parse ? JSON.parse(res[k]) : res[k])
    })
    return out
  }

  // one toJSON batch over states (ygm_tojson_v1); docNames shard the batch over a pool's engines
  _toJsonMany (docNames, states, root, type) {
    const kind = ['map', 'array', 'text'].indexOf(type)
    if (kind < 0 || typeof root !== 'string') throw new TypeError("root: a root name; type: 'map', 'array' or 'text'")
    const eng = this._engine()
    const roots = states.map(() => root)
    return typeof eng.shardOf === 'function' ? eng.toJsonMany(docNames, states, roots, kind) : eng.toJsonMany(states, roots, kind)
  }

  /**
   * versionSharedJson(entries, { root, type, parse }): restoreVersions(entries) followed by one toJSON batch over the
   * fulfilled results, settled per entry as versionJson is (a refused version is rejected with the engine's error and
   * named in `unserialized`).  root, type: as sharedJsonOf's.
   */
  async versionSharedJson (entries, { root = 'default', type = 'map', parse = false } = {}) {
    const out = await this.restoreVersions(entries)
    const ok = out.map((r, i) => r.status === 'fulfilled' ? i : -1).filter(i => i >= 0)
    if (!ok.length) return out
    const res = await this._toJsonMany(ok.map(i => entries[i].documentName), ok.map(i => out[i].value), root, type)
    ok.forEach((i, k) => {
      if (res[k] instanceof Error) {
        this.unserialized.push({ documentName: entries[i].documentName, code: res[k].code || String(res[k]) })
        out[i] = { status: 'rejected', reason: res[k] }
      } else out[i] = { status: 'fulfilled', value: parse ? JSON.parse(res[k]) : res[k] }
    })
    return out
  }

  async onConfigure () { this._engine() }

  /** fetch -> (GPU merge of snapshot + log rows) -> Y.applyUpdate, as Database.onLoadDocument (Database.ts:44-50) */
  async onLoadDocument (data) {
    const [fetched] = await this.store.fetchMany([data])
    let state = null
    if (Array.isArray(fetched)) {
      const parts = fetched.filter(Boolean)
      state = parts.length === 0 ? null : parts.length === 1 ? parts[0] : await this._engine().mergeUpdates(parts, data.documentName)
    } else if (fetched) state = fetched
    if (state) this._Y().applyUpdate(data.document, state)
    this.docs.set(data.documentName, { base: state, log: new UpdateLog() })
  }

  /**
   * Content added while loading (other extensions' onLoadDocument, a returned Doc,
   * Hocuspocus.ts:357-372) never reaches onChange (the listener is registered after
   * load, :382-391): capture it once here (SURVEY.md §8b log-capture hazard 2) -- only when it
   * adds something (new structs, or deletions the base does not hold: encodeStateAsUpdate always
   * carries the whole delete set).  From here on every update of the document is captured by a
   * synchronous Y.Doc 'update' listener, not by onChange: Hocuspocus runs onChange through the
   * extension promise chain (Hocuspocus.ts:263, 465-479), where an earlier extension that throws or
   * awaits I/O would drop or delay it.
   */
  async afterLoadDocument (data) {
    const Y = this._Y()
    const entry = this.docs.get(data.documentName) || { base: null, log: new UpdateLog() }
    this.docs.set(data.documentName, entry)
    const baseSV = entry.base ? Y.encodeStateVectorFromUpdate(entry.base) : new Uint8Array([0])
    const missing = Y.encodeStateAsUpdate(data.document, baseSV)
    if (await addsToBase(this._engine(), missing, entry.base, data.documentName)) entry.log.push(missing)
    if (entry.doc && entry.onUpdate) entry.doc.off('update', entry.onUpdate)
    entry.doc = data.document
    this._gcOf(data.documentName, data.document)
    entry.onUpdate = update => entry.log.push(update)
    data.document.on('update', entry.onUpdate)
  }

  /** every post-load update, whatever its origin (Hocuspocus.ts:263; hazard 1): captured by the
   * document listener of afterLoadDocument; onChange only covers a host that never ran that hook */
  async onChange (data) {
    let entry = this.docs.get(data.documentName)
    if (entry && entry.onUpdate) return
    if (!entry) { entry = { base: null, log: new UpdateLog() }; this.docs.set(data.documentName, entry) }
    entry.log.push(data.update)
  }

  /** store = mergeUpdates([base, ...log]) on the GPU, then the same store payload shape (Database.ts:55-60) */
  async onStoreDocument (data) {
    const entry = this.docs.get(data.documentName) || { base: null, log: new UpdateLog() }
    this.docs.set(data.documentName, entry)
    const taken = entry.log.length
    const nparts = (entry.base ? 1 : 0) + taken
    let state
    // updates the stored state holds: the `taken` ones, or -- when the state is the live document's
    // encodeStateAsUpdate -- every update captured up to that synchronous call (updates that arrive
    // while storeMany is pending are not in it and stay in the log)
    let cut = taken
    if (nparts === 0) { state = this._Y().encodeStateAsUpdate(data.document); cut = entry.log.length } // nothing captured: extension-database's bytes
    else if (nparts === 1) state = entry.base || new Uint8Array(entry.log.toArray(1)[0])   // (a copy: the log's buffer is reused)
    else {
      try {
        // the captured updates go to the batch as one packed range (UpdateLog): one copy per document
        const job = { head: entry.base ? [entry.base] : [], ...entry.log.packed(taken) }
        const eng = this._engine()
        state = await (eng.mergePacked ? eng.mergePacked(job, data.documentName) : eng.mergeUpdates(job.head.concat(entry.log.toArray(taken)), data.documentName))
        if (this.normalize && state.byteLength <= this.normalizeMaxBytes) state = await this._normalize(state, data.documentName, this._gcOf(data.documentName, data.document))
        else if (this.normalize) this.sizeSkipped++
      } catch (e) {
        // a document the engine refuses (content yjs would re-encode, YGM_ENONCANON; a corrupt stored
        // base): unless configured to throw, store what extension-database stores for it -- the live
        // document's Y.encodeStateAsUpdate (Database.ts:58) -- so it keeps persisting.  Anything else (the
        // device, memory, a rejected batch) rejects the hook.
        if (!isRefusal(e) || this.configuration.onRefused === 'throw') throw e
        this.refused.push({ documentName: data.documentName, code: e.code || String(e) })
        state = this._Y().encodeStateAsUpdate(data.document)
        cut = entry.log.length
      }
    }
    // engine results are views into one buffer per batch: keep a copy of exactly this document's bytes, so
    // the long-lived base (and the stored Buffer) do not pin the whole batch's result buffer
    if (state.byteLength !== state.buffer.byteLength) state = new Uint8Array(state)
    await this.store.storeMany([{ payload: data, state: Buffer.from(state.buffer, state.byteOffset, state.byteLength) }])
    // the stored state becomes the new base (under the document's saveMutex, Hocuspocus.ts:427)
    entry.base = state
    entry.log.drop(cut)
  }

  // the doc-normalized snapshot of a merged state (gc false: of a Y.Doc({ gc: false }), deleted content kept); outside
  // the kernel's envelope the merge is kept
  async _normalize (state, documentName, gc = true) {
    try {
      const eng = this._engine()
      if (gc !== false) return await eng.snapshot(state, documentName)
      return await (typeof eng.shardOf === 'function' ? eng.snapshot(state, documentName, { gc: false }) : eng.snapshot(state, { gc: false }))
    } catch (e) {
      if (e && e.code === 'EUNSUPPORTED') { this.unnormalized.push({ documentName, code: e.code }); return state }
      throw e
    }
  }

  async afterUnloadDocument (data) {
    const entry = this.docs.get(data.documentName)
    if (entry && entry.doc && entry.onUpdate) entry.doc.off('update', entry.onUpdate)
    this.docs.delete(data.documentName)
  }

  async onDestroy () { if (this.engine && !this.configuration.engine) this.engine.close(); this.engine = null }
}

// per-document statuses (the batch ran; this document's input was refused), as opposed to batch failures
const REFUSALS = new Set(['EMALFORMED', 'ERANGE', 'ENONCANON', 'ESURROGATE', 'EDEPTH'])
function isRefusal (e) { return !!e && REFUSALS.has(e.code) }

// does `missing` (encodeStateAsUpdate(doc, baseSV)) add structs, or deletions that `base` does not hold?
// Without structs its delete set is the document's whole delete set: it adds nothing iff merging it
// into the base leaves the base's (sorted, merged) delete set unchanged -- decided by two engine merges.
async function addsToBase (engine, missing, base, name) {
  if (missing.length > 0 && missing[0] !== 0) return true                  // struct blocks
  if (missing.length === 2 && missing[1] === 0) return false               // nothing at all
  if (!base) return true
  const [withIt, without] = await Promise.all([engine.mergeUpdates([base, missing], name), engine.mergeUpdates([base, Uint8Array.from([0, 0])], name)])
  return Buffer.compare(Buffer.from(withIt), Buffer.from(without)) !== 0
}

module.exports = { GpuMerge, DocumentStore, isRefusal, GpuEngine, GpuEnginePool, SyncResponder, RedisFanout, UpdateLog, fnv1a64, YgmError }
