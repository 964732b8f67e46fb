'use strict'
// Every field of a document as one object, through the extension: node test/json_fields.js --cpu|--gpu
//  --cpu : GpuMerge over an engine double built from the bundled yjs; checks what the extension asks of the engine
//          (field null / [] / string[]: one jsonFieldsMany call; a string field, and no field at all: jsonMany as before)
//  --gpu : the same through the N-API addon's jsonFields entry (compat135: the bundle is yjs 13.5.16), string for
//          string against yjs
// A live document with three fragment roots ('default', 'sidebar' and '2') and a flat Y.Text document: jsonOf with
// field null equals the reference's fromYdoc(document) over the state the extension holds (tools/json_fields_corpus.js
// restates it); with an array it equals fromYdoc(document, names); with no field it is the single root as before;
// versionJson with field null gives each version's keyed object; the Y.Text document is left out and named.
const path = require('path')
const assert = require('assert')
const { GpuMerge, DocumentStore } = require('../src/index.js')

const mode = process.argv.includes('--gpu') ? 'gpu' : 'cpu'
const TOOLS = path.join(__dirname, '..', '..', '..', 'tools')
const Y = require(path.join(TOOLS, 'yjs_bundle.js')).load()   // the test oracle: yjs from the image's bundle
const { jsonOf, Refuse } = require(path.join(TOOLS, 'json_corpus.js'))
const { fieldsOf } = require(path.join(TOOLS, 'json_fields_corpus.js'))   // [status, JSON.stringify(fromYdoc(doc, fields))]

const CODES = { 1: 'EMALFORMED', 3: 'ENONCANON', 8: 'EINVAL', 9: 'EUNSUPPORTED' }
const load = (state, gc) => { const d = new Y.Doc({ gc }); Y.applyUpdate(d, state); return d }
const isNoGc = o => o === 1 || o === true || !!(o && o.gc === false)
const yjsRestore = (state, version, gc) => Y.encodeStateAsUpdate(Y.createDocFromSnapshot(load(state, false), Y.decodeSnapshot(version), new Y.Doc({ gc })))
const restoreOr = (s, v, gc) => { try { return yjsRestore(s, v, gc) } catch (e) { return Object.assign(new Error(String(e.message)), { code: 'EINVAL' }) } }
const jsonOr = (state, name) => { try { return jsonOf(load(state, true), name) } catch (e) { if (!(e instanceof Refuse)) throw e; return Object.assign(new Error('refused'), { code: 'EUNSUPPORTED' }) } }
const fieldsOr = (state, fields) => { const [st, text] = fieldsOf(state, fields === undefined ? null : fields); return st === 0 ? text : Object.assign(new Error('refused'), { code: CODES[st] }) }
const want = (state, fields) => { const [st, text] = fieldsOf(state, fields); assert.strictEqual(st, 0); return text }

// test double (never shipped): the engine calls the extension makes, from yjs
class Double {
  constructor () { this.log = [] }
  async mergeUpdates (updates) { return Y.mergeUpdates(updates) }
  async mergeMany (docs) { return docs.map(u => Y.mergeUpdates(u)) }
  async snapshot (update, opts) { return Y.encodeStateAsUpdate(load(update, !(opts && opts.gc === false))) }
  async takeVersionMany (states) { return states.map(s => Y.encodeSnapshot(Y.snapshot(load(s, true)))) }
  async restoreVersionMany (states, versions, opts) { return states.map((s, i) => restoreOr(s, versions[i], !(opts && isNoGc(opts[i])))) }
  async jsonMany (states, names) {
    this.log.push(['jsonMany', states.length, Array.from(names)])
    return states.map((s, i) => jsonOr(s, String(names[i])))
  }
  async jsonFieldsMany (states, fields) {
    this.log.push(['jsonFieldsMany', states.length, Array.from(fields)])
    return states.map((s, i) => fieldsOr(s, fields[i]))
  }
  close () {}
}

class MemoryStore extends DocumentStore {
  constructor () { super(); this.rows = new Map() }
  async fetchMany (payloads) { return payloads.map(p => this.rows.get(p.documentName) || null) }
  async storeMany (entries) { for (const e of entries) this.rows.set(e.payload.documentName, Uint8Array.from(e.state)) }
}

async function openDoc (ext, name, gc, id) {
  const document = new Y.Doc({ gc })
  document.clientID = id
  document.name = name
  const payload = { document, documentName: name, context: {}, requestParameters: new Map() }
  await ext.onLoadDocument(payload)
  await ext.afterLoadDocument(payload)
  return payload
}

function makeEngine () {
  if (mode === 'cpu') return new Double()
  const { GpuEngine } = require('../src/engine.js')
  return new GpuEngine({ device: 0, batchWindowMs: 5, compat135: true })
}

function block (frag, at, tag, s, level) {
  const e = new Y.XmlElement(tag)
  frag.insert(at, [e])
  if (tag === 'heading') e.setAttribute('level', level)
  const t = new Y.XmlText()
  e.insert(0, [t])
  t.insert(0, s)
  return t
}

test_('jsonOf and versionJson with field null, an array, and the untouched string default; a refused document is named', async () => {
  const engine = makeEngine()
  const ext = new GpuMerge({ engine, store: new MemoryStore(), Y })
  try {
    const x = await openDoc(ext, 'tiptap', false, 41)
    const f = await openDoc(ext, 'flat', false, 42)
    const vx = []
    block(x.document.getXmlFragment('default'), 0, 'heading', 'Body "one"', 1)
    block(x.document.getXmlFragment('sidebar'), 0, 'paragraph', 'A note 😀 beside it.')
    f.document.getText('default').insert(0, 'flat text')
    vx.push((await ext.takeVersions(['tiptap'])).get('tiptap'))
    block(x.document.getXmlFragment('2'), 0, 'paragraph', 'An index-named field.')
    block(x.document.getXmlFragment('default'), 1, 'paragraph', 'More body.').format(0, 4, { bold: true })
    vx.push((await ext.takeVersions(['tiptap'])).get('tiptap'))
    const held = (await ext._statesOf(['tiptap']))[0]   // the state the extension serializes: its key order is this state's doc.share order

    // field: null -- fromYdoc(document): every field, index keys first
    const all = await ext.jsonOf(['tiptap', 'missing', 'flat'], { field: null })
    assert.deepStrictEqual(Array.from(all.keys()), ['tiptap'])
    assert.strictEqual(all.get('tiptap'), want(held, null))
    assert.deepStrictEqual(Object.keys(JSON.parse(all.get('tiptap'))), ['2', 'default', 'sidebar'])
    assert.deepStrictEqual(ext.unserialized, [{ documentName: 'flat', code: 'EUNSUPPORTED' }])
    ext.unserialized.length = 0
    assert.strictEqual((await ext.jsonOf(['tiptap'], { field: [] })).get('tiptap'), want(held, null))
    const live = d => ({ 2: JSON.parse(jsonOf(d, '2')), default: JSON.parse(jsonOf(d, 'default')), sidebar: JSON.parse(jsonOf(d, 'sidebar')) })
    assert.deepStrictEqual((await ext.jsonOf(['tiptap'], { field: null, parse: true })).get('tiptap'), live(load(Y.encodeStateAsUpdate(x.document), true)))

    // field: string[] -- fromYdoc(document, names): list order, an absent name, a repeated one
    const list = ['sidebar', 'absent', 'default', 'sidebar']
    const some = (await ext.jsonOf(['tiptap'], { field: list })).get('tiptap')
    assert.strictEqual(some, want(held, list))
    assert.strictEqual(some, '{"sidebar":' + jsonOf(load(held, true), 'sidebar') + ',"absent":{"type":"doc","content":[]},"default":' + jsonOf(load(held, true), 'default') + '}')
    // a __proto__ field: refused and named, the caller keeps its yjs path
    assert.strictEqual((await ext.jsonOf(['tiptap'], { field: ['default', '__proto__'] })).size, 0)
    assert.deepStrictEqual(ext.unserialized, [{ documentName: 'tiptap', code: 'EUNSUPPORTED' }])
    ext.unserialized.length = 0
    await assert.rejects(ext.jsonOf(['tiptap'], { field: 7 }), TypeError)

    // no field, and a string field: one root, the path of before
    const one = (await ext.jsonOf(['tiptap'])).get('tiptap')
    assert.strictEqual(one, jsonOf(load(held, true), 'default'))
    assert.strictEqual((await ext.jsonOf(['tiptap'], { field: undefined })).get('tiptap'), one)
    assert.strictEqual((await ext.jsonOf(['tiptap'], { field: 'sidebar' })).get('tiptap'), jsonOf(load(held, true), 'sidebar'))
    if (mode === 'cpu') {
      assert.deepStrictEqual(engine.log, [['jsonFieldsMany', 2, [null, null]], ['jsonFieldsMany', 1, [[]]], ['jsonFieldsMany', 1, [null]],
        ['jsonFieldsMany', 1, [list]], ['jsonFieldsMany', 1, [['default', '__proto__']]],
        ['jsonMany', 1, ['default']], ['jsonMany', 1, ['default']], ['jsonMany', 1, ['sidebar']]])
      engine.log.length = 0
    }

    // versionJson with field null: each version's keyed object (the first version has no '2' yet)
    const entries = [{ documentName: 'tiptap', version: vx[1] }, { documentName: 'gone', version: vx[0] }, { documentName: 'tiptap', version: vx[0] }]
    const res = await ext.versionJson(entries, { field: null, parse: true })
    assert.deepStrictEqual(res.map(r => r.status), ['fulfilled', 'rejected', 'fulfilled'])
    const at = v => Y.createDocFromSnapshot(x.document, Y.decodeSnapshot(v))
    assert.deepStrictEqual(res[0].value, live(at(vx[1])))
    assert.deepStrictEqual(Object.keys(res[2].value).sort(), ['default', 'sidebar'])
    assert.deepStrictEqual(res[2].value.sidebar, JSON.parse(jsonOf(at(vx[0]), 'sidebar')))
    const text = await ext.versionJson(entries.slice(0, 1), { field: ['2'] })
    assert.strictEqual(text[0].value, '{"2":' + jsonOf(at(vx[1]), '2') + '}')
    assert.strictEqual((await ext.versionJson(entries.slice(0, 1)))[0].value, jsonOf(at(vx[1]), 'default'))
    if (mode === 'cpu') assert.deepStrictEqual(engine.log, [['jsonFieldsMany', 2, [null, null]], ['jsonFieldsMany', 1, [['2']]], ['jsonMany', 1, ['default']]])
  } finally { engine.close() }
})

if (mode === 'gpu') {
  test_('the addon and the pool: objects in caller order, refusals alone, names as strings or bytes', async () => {
    const { GpuEngine, GpuEnginePool, encodeFields } = require('../src/engine.js')
    const engine = new GpuEngine({ device: 0, compat135: true })
    try {
      const d = new Y.Doc(); d.clientID = 9
      block(d.getXmlFragment('default'), 0, 'heading', 'nested', 3)
      block(d.getXmlFragment('tëxt'), 0, 'paragraph', 'héllo')
      const u = Y.encodeStateAsUpdate(d)
      const t = new Y.Doc(); t.clientID = 10
      t.getText('plain').insert(0, 'a text root')
      const ut = Y.encodeStateAsUpdate(t)
      assert.strictEqual(typeof engine.jsonFieldsMany, 'function')
      assert.deepStrictEqual(Array.from(encodeFields(['a', Buffer.from('bc')])), [1, 97, 2, 98, 99])
      assert.strictEqual(encodeFields(['x'.repeat(128)]).length, 130)
      const E = '{"type":"doc","content":[]}'
      const r = await engine.jsonFieldsMany([u, u.slice(0, u.length - 4), ut, u, u, u, Uint8Array.from([0, 0])],
        [null, null, undefined, [Buffer.from('tëxt'), 'absent'], ['default', '__proto__'], [], ['only']])
      assert.strictEqual(r[0], want(u, null))
      assert.ok(r[1] instanceof Error && r[1].code === 'EMALFORMED')
      assert.ok(r[2] instanceof Error && r[2].code === 'EUNSUPPORTED')
      assert.strictEqual(r[3], '{"tëxt":' + jsonOf(load(u, true), 'tëxt') + ',"absent":' + E + '}')
      assert.ok(r[4] instanceof Error && r[4].code === 'EUNSUPPORTED')
      assert.strictEqual(r[5], r[0])
      assert.strictEqual(r[6], '{"only":' + E + '}')
      assert.deepStrictEqual(await engine.jsonFieldsMany([], []), [])
      await assert.rejects(engine.jsonFieldsMany([u], []), x => x.code === 'EINVAL')
      const pool = new GpuEnginePool({ makeEngine: () => engine, devices: [0] })
      assert.deepStrictEqual(await pool.jsonFieldsMany(['a', 'b'], [u, u], [null, ['absent']]), [r[0], '{"absent":' + E + '}'])
    } finally { engine.close() }
  })
}

function test_ (name, fn) { (test_.all = test_.all || []).push({ name, fn }) }

;(async () => {
  let failed = 0
  for (const t of test_.all) {
    try { await t.fn(); console.log('ok   ' + t.name) } catch (e) { failed++; console.log('FAIL ' + t.name + '\n' + (e && e.stack || e)) }
  }
  console.log(failed ? failed + ' failed' : test_.all.length + ' passed (' + mode + ')')
  process.exit(failed ? 1 : 0)
})()
